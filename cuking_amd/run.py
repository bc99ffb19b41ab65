"""Multi-GPU driver with the reference's CLI surface (cuking.cu:27-52):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \\
        --master-addr 127.0.0.1 --master-port 29500 -m cuking_amd.run \\
        --input-uri in/ --output-uri out/ --kin-threshold 0.05

One process per GPU.  Rank 0 reads `metadata.json` + `*.parquet`, packs the
bitset through the C ABI (`cuking_pack_host`, reader threads like
cuking.cu:550-553) -- or, with `--bed-uri PREFIX`, streams a PLINK `.bed` to its
GPU and transposes it there (`KingContext.load_bed`) --, optionally drops sites
by call rate, minor allele frequency / count, the Hardy-Weinberg exact test or a list
(`--site-min-call-rate`, `--site-min-maf`, `--site-min-mac`, `--site-hwe-p`, `--site-keep-uri`:
counts, test and compaction on the GPU, csrc/king_site_qc.hip and csrc/king_hwe.hip) and thins the rest by LD (`--site-ld-window`, `--site-ld-r2`:
csrc/king_ld.hip), the bitset goes to the other GPUs by the staged RCCL
broadcast of `cuking_amd.dist`, every rank evaluates its band of the pair
space, rank 0 gathers, sorts and writes `part-<shard>.snappy.parquet` with the
reference's schema (cuking.cu:767-870).  `--split-factor/--shard-index` select a
block exactly like the reference; the GPUs of the node share that block's work
(this replaces the one-VM-per-shard fan-out of cloud_batch_submit.py:45,73).
With a single process (no torchrun) it is the one-GPU path.

The single-GPU drop-in without Python is the C++ binary `cuking_amd/bin/cuking`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="cuking_amd.run", allow_abbrev=False)

    def flag(name, **kw):  # accept --kin-threshold and --kin_threshold
        ap.add_argument(f"--{name}", f"--{name.replace('-', '_')}",
                        dest=name.replace("-", "_"), **kw)

    flag("input-uri", default="")
    flag("bed-uri", default="",
         help="PREFIX of a PLINK 1 binary genotype set (PREFIX.bed / .bim / .fam, variant-major) "
              "to read instead of --input-uri: the dense 2-bit file goes to the GPU as it is and "
              "is transposed into the bitset there; sample ids come from the .fam")
    flag("output-uri", default="")
    flag("requester-pays-project", default="")
    flag("num-reader-threads", type=int, default=36)
    flag("max-results", type=int, default=10 << 20)
    flag("kin-threshold", type=float, default=0.0884)
    flag("split-factor", type=int, default=1)
    flag("shard-index", type=int, default=0)
    flag("chunks", type=int, default=8)
    flag("variant", type=int, default=-1,
         help="tiled kernel variant (default: the library's, 7 = one-product filter + exact "
              "recount; 6 = four products for every pair, the choice when more than ~10 %% of "
              "the calls are missing; same records either way)")
    flag("synthetic", default="",
         help="N,M[,seed]: instead of reading --input-uri, generate the synthetic cohort of "
              "cuking_amd.synth on the GPU (BASELINE configs without their 10^9..10^11-row "
              "Parquet form)")
    flag("synthetic-model", default="",
         help="cohort model of --synthetic: baseline (default), exome or admixed "
              "(csrc/synth.hip holds the specification)")
    flag("kin-matrix-uri", default="",
         help="also write the block's dense kinship matrix -- the float32 kinship of EVERY "
              "pair, no threshold -- to this .npy file ([NumRows, NumCols]; a diagonal block "
              "symmetric with its diagonal).  One process only; the matrix must fit the GPU "
              "beside the bitset (4 B x NumRows x NumCols: use --split-factor otherwise)")
    flag("kin-summary-uri", default="",
         help="also write the block's kinship summary -- the histogram of the float32 kinship "
              "of EVERY pair and every sample's nearest relative, no matrix and no threshold "
              "-- to this .npz file (hist, lo, hi, bins, best_kin, best_partner).  One process "
              "only")
    flag("kin-summary-bins", default="",
         help="LO,HI,N: the histogram of --kin-summary-uri (default -1,0.5,1536; N + 3 slots: "
              "below LO, the N bins, from HI on, NaN); write --kin-summary-bins=-0.25,0.25,64 "
              "when LO is negative")
    flag("relative-counts-uri", default="",
         help="also write the block's relative counts -- per sample, the number of partners "
              "whose kinship falls in each band of a few thresholds, no records and nothing "
              "that can overflow -- to this .npz file (bands, thresholds, samples).  One "
              "process only")
    flag("relative-thresholds", default="",
         help="A,B,...: the 1 to 8 strictly ascending thresholds of --relative-counts-uri "
              "(default: the KING cut-offs 0.0442,0.0884,0.177,0.354); write "
              "--relative-thresholds=-0.1,0.1 when the first is negative")
    flag("unrelated-uri", default="",
         help="also write the unrelated set and the families of the records' graph -- which "
              "samples to keep so that no two kept samples are related, computed on the GPU "
              "from the records -- to this .npz file (keep, family, samples, threshold).  One "
              "process and --split-factor 1 only")
    flag("unrelated-priority", default="",
         help="a .npy file of one float32 priority per sample for --unrelated-uri: the higher "
              "priority is kept first, among equals the earlier sample (default: fewer "
              "relatives first)")
    flag("unrelated-threshold", type=float, default=None,
         help="records with kin above this are the edges of --unrelated-uri (default: "
              "--kin-threshold; not below it)")
    flag("site-min-call-rate", type=float, default=None,
         help="site QC before anything is computed: keep the sites whose share of called "
              "genotypes is at least this (0..1).  Any of --site-min-call-rate, --site-min-maf, "
              "--site-min-mac, --site-hwe-p and --site-keep-uri makes the run count the genotypes per site on "
              "the GPU, drop the sites that fail (and those without a called genotype) and "
              "compact the bitset there; records and every side output then come from the kept "
              "sites.  One process and --split-factor 1 only")
    flag("site-min-maf", type=float, default=None,
         help="site QC: keep the sites whose minor allele frequency among the called genotypes "
              "is at least this (0..1; above 0.5 nothing passes)")
    flag("site-min-mac", type=int, default=None,
         help="site QC: keep the sites whose minor allele count is at least this (1 drops the "
              "monomorphic sites)")
    flag("site-hwe-p", type=float, default=None,
         help="site QC: keep the sites whose Hardy-Weinberg exact test p-value (Wigginton et "
              "al. 2005, computed on the GPU from the cohort's genotype counts: plink --hwe) is "
              "at least this (0..1, e.g. 1e-6); applied with the rule, before LD pruning")
    ap.add_argument("--site-hwe-midp", "--site_hwe_midp", dest="site_hwe_midp",
                    action="store_true",
                    help="site QC: --site-hwe-p uses the mid-p form of the test (half the "
                         "observed table's probability leaves the tail); needs --site-hwe-p")
    flag("site-keep-uri", default="",
         help="site QC: a .npy file of one bool / uint8 per site, ANDed with the rule -- an "
              "LD-pruned site list, a region")
    flag("site-qc-uri", default="",
         help="also write the site QC report of the INPUT cohort to this .npz file "
              "(site_counts [sites, 4] = hom-ref, het, hom-var, missing; keep; sample_counts "
              "[samples, 4]; samples; min_call_rate, min_maf, min_mac; with --site-hwe-p also "
              "hwe_p, min_hwe_p and hwe_midp).  Alone it only reports: "
              "nothing is filtered.  One process and --split-factor 1 only")
    flag("site-ld-window", type=int, default=None,
         help="LD pruning after the site QC rule, on the GPU: among the sites within a window "
              "of this many variants (default 50; pairs up to W - 1 apart, never across the "
              "chromosomes of a --bed-uri's .bim) no two kept sites have an r^2 above "
              "--site-ld-r2; of a correlated pair the site with the higher minor allele "
              "frequency stays.  Any of --site-ld-window, --site-ld-r2 and --site-ld-uri turns "
              "it on.  One process and --split-factor 1 only")
    flag("site-ld-r2", type=float, default=None,
         help="LD pruning: the r^2 threshold (0..1, default 0.2)")
    flag("site-ld-uri", default="",
         help="LD pruning: also write its report to this .npz file (keep over the sites that "
              "entered the pruning, kept_index in input-site numbering, num_edges, window, r2)")
    flag("pca-uri", default="",
         help="also write the principal components of the standardized genotypes -- fitted on "
              "the samples --pca-fit selects, EVERY sample projected, on the bitset site QC and "
              "LD pruning left (cuking_amd/pca.py) -- to this .npz file (eigenvalues, scores, "
              "loadings, allele_freq, sites_used, fit, samples).  One process and "
              "--split-factor 1 only")
    flag("pca-components", type=int, default=None,
         help="the number of components of --pca-uri (default 10)")
    flag("pca-fit", default="",
         help="the samples the components of --pca-uri are fitted on: all (default) or "
              "unrelated, the kept samples of this run's --unrelated-uri")
    flag("pcrelate-uri", default="",
         help="also write the PC-Relate kinship matrix of the whole cohort -- ancestry-adjusted "
              "with the scores and the fit of this run's --pca-uri (cuking_amd/pcrelate.py) -- to "
              "this float32 .npy file [samples, samples].  Needs --pca-uri; one process and "
              "--split-factor 1 only")
    flag("pcrelate-pairs-uri", default="",
         help="also re-score this run's records with PC-Relate -- no matrix: kin, k0, k1, k2, "
              "ibs0, sites and the relationship code of every record's pair, ancestry-adjusted "
              "with the scores and the fit of this run's --pca-uri -- and write them to this .npz "
              "(with sample_i, sample_j, inbreeding, samples).  Needs --pca-uri; one process and "
              "--split-factor 1 only")
    flag("pcrelate-records-uri", default="",
         help="also scan ALL pairs of the cohort with PC-Relate -- no matrix, ancestry-adjusted "
              "with the scores and the fit of this run's --pca-uri -- and write the pairs whose "
              "kinship is above --pcrelate-min-kinship to this .npz: sample_i, sample_j, kin, "
              "then k0, k1, k2, ibs0, sites, kin_pairs and the relationship code of those pairs "
              "(with samples, min_kinship, num_records).  Needs --pca-uri; one process and "
              "--split-factor 1 only")
    flag("ibd-segments-uri", default="",
         help="also scan this run's records for IBD segments -- the runs of at least "
              "--ibd-min-sites sites without an opposite homozygote (IBD1) and without a "
              "difference (IBD2), no allele frequencies and no principal components involved "
              "(cuking_amd/ibd.py) -- and write them to this .npz: sample_i, sample_j, segments1, "
              "segments2, length1, length2, longest1, longest2, total_length, pi1, pi2, kin_ibd "
              "and the relationship code of every record's pair (with samples, min_sites, "
              "min_length).  The scan runs on the bitset the records were computed on, after "
              "site QC and LD pruning: LD pruning thins the markers a segment is counted in, so "
              "choose --ibd-min-sites for the markers that are left.  With --bed-uri the "
              "chromosomes and base-pair positions of the .bim bound and measure the segments; "
              "otherwise there is one group and the position is the site index.  One process "
              "and --split-factor 1 only")
    flag("ibd-min-sites", type=int, default=None,
         help="the fewest sites of a segment of --ibd-segments-uri (default 512; at least 64)")
    flag("ibd-min-length", type=int, default=None,
         help="the least length of a segment of --ibd-segments-uri, in the .bim's positions "
              "(default 0)")
    flag("ibd-bridge-sites", type=int, default=None,
         help="--ibd-segments-uri forgives isolated genotyping errors: two runs of at least this "
              "many sites on either side of one break site of a chromosome count as one "
              "segment (0, or at least 64; default: no bridging).  Adds bridge_sites, bridged1 "
              "and bridged2 (the bridged breaks inside each record's counted segments) to the "
              "file")
    flag("ibd-segment-list", action="store_true",
         help="--ibd-segments-uri also writes the segments themselves: segment_pair (the "
              "record's number), segment_kind, segment_first_site, segment_last_site (site "
              "numbers among the input's sites), sorted")
    flag("ibd-scan-uri", default="",
         help="also scan EVERY pair of the cohort for IBD segments, without a list: the pairs "
              "with a run of at least --ibd-scan-min-sites sites without an opposite homozygote "
              "(IBD1) whose summed length reaches --ibd-scan-min-total (cuking_amd/ibd.py, "
              "ibd_scan) -- relatives whose kinship lies below this run's threshold included -- "
              "written to this .npz: sample_i, sample_j, segments1, segments2, length1, length2, "
              "longest1, longest2, total_length, pi1, pi2, kin_ibd and relationship, one entry "
              "per pair found, by (sample_i, sample_j) (with samples, min_sites, min_length, "
              "min_total).  The scan runs on the bitset the records were computed on, after "
              "site QC and LD pruning, and takes chromosomes and base-pair positions from the "
              ".bim under --bed-uri exactly as --ibd-segments-uri does.  One process and "
              "--split-factor 1 only")
    flag("ibd-scan-min-sites", type=int, default=None,
         help="the fewest sites of a segment of --ibd-scan-uri (default 512; at least 64)")
    flag("ibd-scan-min-length", type=int, default=None,
         help="the least length of a segment of --ibd-scan-uri, in the .bim's positions "
              "(default 0)")
    flag("ibd-scan-min-total", type=int, default=None,
         help="the least summed length of a pair's IBD1 segments for --ibd-scan-uri to keep the "
              "pair (default 0: every pair with a segment)")
    flag("roh-uri", default="",
         help="also scan every sample of this run for runs of homozygosity -- the runs of at "
              "least --roh-min-sites sites without a heterozygous call, no allele frequencies "
              "and no principal components involved (cuking_amd/roh.py) -- and write them to "
              "this .npz: sample, segments, length, longest, bridged, froh (length over "
              "total_length: the inbreeding estimate F_ROH), total_length (with samples, "
              "min_sites, min_length, bridge_sites).  The scan runs on the bitset the records "
              "were computed on, after site QC and LD pruning, and takes chromosomes and "
              "base-pair positions from the .bim under --bed-uri exactly as "
              "--ibd-segments-uri does.  One process and --split-factor 1 only")
    flag("roh-min-sites", type=int, default=None,
         help="the fewest sites of a run of --roh-uri (default 512; at least 64)")
    flag("roh-min-length", type=int, default=None,
         help="the least length of a run of --roh-uri, in the .bim's positions (default 0)")
    flag("roh-bridge-sites", type=int, default=None,
         help="--roh-uri forgives isolated heterozygous calls (genotyping errors): two runs of "
              "at least this many sites on either side of one het of a chromosome count as one "
              "run (0, or at least 64; default 0: no bridging)")
    flag("roh-segment-list", action="store_true",
         help="--roh-uri also writes the runs themselves: seg_sample, seg_first_site, "
              "seg_last_site (site numbers among the input's sites), sorted")
    flag("mendel-uri", default="",
         help="also count the Mendelian errors of trios and duos -- the sites at which a child's "
              "genotype cannot come from its parents', by the eight autosomal codes of plink "
              "--mendel and hl.mendel_errors (cuking_amd/mendel.py) -- and write them to this "
              ".npz: child, father, mother (sample numbers, -1 for an absent parent), called, "
              "errors [T, 8], rate (errors over called), per_sample (the errors that implicate "
              "each sample, PLINK's .imendel rule) and samples.  The trios are those the .fam "
              "under --bed-uri declares, or --mendel-trios.  The count runs on the bitset the "
              "records were computed on, after site QC and LD pruning.  One process and "
              "--split-factor 1 only")
    flag("mendel-trios", default="",
         help="the trios of --mendel-uri: a .npy with an integer [T, 3] array of (child, father, "
              "mother) sample numbers, -1 for an absent parent (required unless --bed-uri names a "
              ".fam that declares parents)")
    flag("mendel-site-counts", action="store_true",
         help="--mendel-uri also writes site_errors, the number of listed trios with an error "
              "at each site, and site_index, the sites' numbers among the input's sites")
    flag("pihat-uri", default="",
         help="also scan ALL pairs of the cohort for PI_HAT, the method-of-moments IBD estimate "
              "of PLINK --genome / hl.identity_by_descent (allele frequencies of the cohort's "
              "own samples, after site QC and LD pruning), and write the pairs with PI_HAT above "
              "--pihat-min to this .npz: sample_i, sample_j, pi_hat, z0, z1, z2, ibs0, ibs1, "
              "ibs2 sorted by pair, samples, the model, min_pi_hat, num_records.  Assumes one "
              "homogeneous population.  One process and --split-factor 1 only")
    flag("pihat-min", type=float, default=None,
         help="the threshold of --pihat-uri: pairs with a PI_HAT strictly above it (default "
              "0.0884, the third-degree kinship cut-off doubled)")
    flag("pihat-unbounded", action="store_true",
         help="--pihat-uri without the bounding of z0, z1, z2 to [0, 1]")
    flag("pcrelate-min-kinship", type=float, default=None,
         help="the threshold of --pcrelate-records-uri: pairs with a kinship strictly above it "
              "(default 0.0442, the third-degree cut-off)")
    flag("pcrelate-components", type=int, default=None,
         help="the number of leading components --pcrelate-uri, --pcrelate-pairs-uri and "
              "--pcrelate-records-uri adjust "
              "for (default: all of --pca-components; at most 31)")
    flag("pcrelate-min-maf", type=float, default=None,
         help="--pcrelate-uri, --pcrelate-pairs-uri and --pcrelate-records-uri use the elements "
              "whose "
              "individual-specific allele frequency lies strictly between this and 1 minus this "
              "(default 0.01)")
    return ap.parse_args(argv)


class UsageError(Exception):
    pass


def resolve_uri(uri: str) -> Path:
    if uri.startswith("gs://"):
        raise UsageError(f"Unsupported URI: {uri} (no GCS client in this build; "
                         "pass a local directory or file:// URI)")
    return Path(uri[7:] if uri.startswith("file://") else uri)


def summary_bins(text: str):
    """--kin-summary-bins LO,HI,N -> (lo, hi, n)."""
    if not text:
        return -1.0, 0.5, 1536
    parts = text.split(",")
    try:
        # (as the library sees them: float32)
        lo, hi, n = float(np.float32(parts[0])), float(np.float32(parts[1])), int(parts[2])
        if len(parts) != 3 or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi) or \
                not 1 <= n <= 4096:
            raise ValueError
    except (ValueError, IndexError):
        raise UsageError("--kin_summary_bins expects LO,HI,N with finite LO < HI and "
                         "1 <= N <= 4096") from None
    return lo, hi, n


def relative_thresholds(text: str):
    """--relative-thresholds A,B,... -> the thresholds as the library sees them (float32)."""
    if not text:
        return (0.0442, 0.0884, 0.177, 0.354)
    try:
        thr = np.array([float(x) for x in text.split(",")], dtype=np.float32)
        if not 1 <= thr.size <= 8 or not np.isfinite(thr).all() or not (np.diff(thr) > 0).all():
            raise ValueError
    except ValueError:
        raise UsageError("--relative_thresholds expects 1 to 8 finite, strictly ascending "
                         "values A,B,...") from None
    return tuple(float(t) for t in thr)


def validate(args):  # cuking.cu:437-462
    if args.synthetic_model and not args.synthetic:
        raise UsageError("--synthetic_model needs --synthetic")
    if not args.input_uri and not args.bed_uri and not args.synthetic:
        raise UsageError("No input URI specified: exactly one of --input_uri, --bed_uri and "
                         "--synthetic is required")
    if args.bed_uri and (args.input_uri or args.synthetic):
        raise UsageError("exactly one of --input_uri, --bed_uri and --synthetic is required, "
                         "--bed_uri came with another of them")
    if not args.output_uri:
        raise UsageError("No output URI specified")
    if args.num_reader_threads <= 0:
        raise UsageError("Invalid number of reader threads")
    if args.split_factor <= 0:
        raise UsageError("Invalid split factor")
    if not 0 <= args.shard_index < args.split_factor * (args.split_factor + 1) // 2:
        raise UsageError("Invalid shard index")
    if args.kin_matrix_uri and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise UsageError("--kin_matrix_uri needs one process (one GPU): a dense kinship matrix "
                         "is not assembled from several GPUs; run the shards of a "
                         "--split-factor one after the other instead")
    if args.kin_summary_bins and not args.kin_summary_uri:
        raise UsageError("--kin_summary_bins needs --kin_summary_uri")
    if args.kin_summary_uri and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise UsageError("--kin_summary_uri needs one process (one GPU): summaries are not "
                         "merged across ranks yet")
    summary_bins(args.kin_summary_bins)
    if args.relative_thresholds and not args.relative_counts_uri:
        raise UsageError("--relative_thresholds needs --relative_counts_uri")
    if args.relative_counts_uri and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise UsageError("--relative_counts_uri needs one process (one GPU): relative counts "
                         "are not merged across ranks yet")
    relative_thresholds(args.relative_thresholds)
    if (args.unrelated_priority or args.unrelated_threshold is not None) and \
            not args.unrelated_uri:
        raise UsageError("--unrelated_priority and --unrelated_threshold need --unrelated_uri")
    if args.unrelated_uri and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise UsageError("--unrelated_uri needs one process (one GPU): unrelated sets are not "
                         "merged across ranks yet")
    if args.unrelated_uri and args.split_factor != 1:
        raise UsageError("--unrelated_uri needs --split_factor 1: the unrelated set is a "
                         "property of the whole cohort's records (concatenate the shards' "
                         "record buffers and call unrelated_set instead)")
    unrelated_threshold(args)
    if site_filtering(args) or args.site_qc_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--site_min_call_rate, --site_min_maf, --site_min_mac, --site_hwe_p, "
                             "--site_keep_uri and --site_qc_uri need one process (one GPU): site "
                             "counts are not merged across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--site_min_call_rate, --site_min_maf, --site_min_mac, --site_hwe_p, "
                             "--site_keep_uri and --site_qc_uri need --split_factor 1: a site "
                             "passes or fails on the whole cohort's counts")
    site_rule(args)
    hwe_rule(args)
    if ld_pruning(args):
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--site_ld_window, --site_ld_r2 and --site_ld_uri need one process "
                             "(one GPU): LD edges are not merged across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--site_ld_window, --site_ld_r2 and --site_ld_uri need "
                             "--split_factor 1: r^2 is taken over the whole cohort's samples")
    ld_rule(args)
    if (args.pca_components is not None or args.pca_fit) and not args.pca_uri:
        raise UsageError("--pca_components and --pca_fit need --pca_uri")
    if args.pca_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--pca_uri needs one process (one GPU): the products are not "
                             "merged across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--pca_uri needs --split_factor 1: the components are fitted on the "
                             "whole cohort's bitset")
        if args.pca_fit not in ("", "all", "unrelated"):
            raise UsageError("--pca_fit expects all or unrelated")
        if args.pca_fit == "unrelated" and not args.unrelated_uri:
            raise UsageError("--pca_fit unrelated needs the unrelated set of the same run: pass "
                             "--unrelated_uri as well")
        if args.pca_components is not None and args.pca_components < 1:
            raise UsageError("--pca_components must be at least 1")
    if (args.pcrelate_components is not None or args.pcrelate_min_maf is not None) and \
            not (args.pcrelate_uri or args.pcrelate_pairs_uri or args.pcrelate_records_uri):
        raise UsageError("--pcrelate_components and --pcrelate_min_maf need --pcrelate_uri or "
                         "--pcrelate_pairs_uri")
    if args.pcrelate_pairs_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--pcrelate_pairs_uri needs one process (one GPU): the records are "
                             "not re-scored across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--pcrelate_pairs_uri needs --split_factor 1: the model is fitted "
                             "on the whole cohort's bitset")
        if not args.pca_uri:
            raise UsageError("--pcrelate_pairs_uri needs the principal components of the same "
                             "run: pass --pca_uri as well")
    if (args.ibd_min_sites is not None or args.ibd_min_length is not None or
            args.ibd_segment_list) and not args.ibd_segments_uri:
        raise UsageError("--ibd_min_sites, --ibd_min_length and --ibd_segment_list need "
                         "--ibd_segments_uri")
    if args.ibd_bridge_sites is not None:
        if not args.ibd_segments_uri:
            raise UsageError("--ibd_bridge_sites needs --ibd_segments_uri")
        if args.ibd_bridge_sites != 0 and not IBD_MIN_SITES <= args.ibd_bridge_sites < 1 << 32:
            raise UsageError(f"--ibd_bridge_sites must be 0 or at least {IBD_MIN_SITES} (and "
                             "below 2^32): shorter runs lie inside one 64-site word, which the "
                             "scan does not enumerate")
    if args.ibd_segments_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--ibd_segments_uri needs one process (one GPU): the records are "
                             "not scanned across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--ibd_segments_uri needs --split_factor 1: it scans the records of "
                             "the whole cohort's bitset")
        if args.ibd_min_sites is not None and args.ibd_min_sites < IBD_MIN_SITES:
            raise UsageError(f"--ibd_min_sites must be at least {IBD_MIN_SITES}: shorter runs "
                             "lie inside one 64-site word, which the scan does not enumerate")
        if args.ibd_min_length is not None and not 0 <= args.ibd_min_length < 1 << 32:
            raise UsageError("--ibd_min_length must be in [0, 2^32)")
    if (args.ibd_scan_min_sites is not None or args.ibd_scan_min_length is not None or
            args.ibd_scan_min_total is not None) and not args.ibd_scan_uri:
        raise UsageError("--ibd_scan_min_sites, --ibd_scan_min_length and --ibd_scan_min_total "
                         "need --ibd_scan_uri")
    if args.ibd_scan_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--ibd_scan_uri needs one process (one GPU): the pairs are not "
                             "scanned across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--ibd_scan_uri needs --split_factor 1: it scans every pair of the "
                             "whole cohort's bitset")
        if args.ibd_scan_min_sites is not None and \
                not IBD_MIN_SITES <= args.ibd_scan_min_sites < 1 << 32:
            raise UsageError(f"--ibd_scan_min_sites must be at least {IBD_MIN_SITES} (and below "
                             "2^32): shorter runs lie inside one 64-site word, which the scan "
                             "does not enumerate")
        if args.ibd_scan_min_length is not None and not 0 <= args.ibd_scan_min_length < 1 << 32:
            raise UsageError("--ibd_scan_min_length must be in [0, 2^32)")
        if args.ibd_scan_min_total is not None and not 0 <= args.ibd_scan_min_total < 1 << 64:
            raise UsageError("--ibd_scan_min_total must be in [0, 2^64)")
    if (args.roh_min_sites is not None or args.roh_min_length is not None or
            args.roh_bridge_sites is not None or args.roh_segment_list) and not args.roh_uri:
        raise UsageError("--roh_min_sites, --roh_min_length, --roh_bridge_sites and "
                         "--roh_segment_list need --roh_uri")
    if args.roh_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--roh_uri needs one process (one GPU): the samples are not "
                             "scanned across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--roh_uri needs --split_factor 1: it scans the samples of the "
                             "whole cohort's bitset")
        if args.roh_min_sites is not None and not IBD_MIN_SITES <= args.roh_min_sites < 1 << 32:
            raise UsageError(f"--roh_min_sites must be at least {IBD_MIN_SITES} (and below "
                             "2^32): shorter runs lie inside one 64-site word, which the scan "
                             "does not enumerate")
        if args.roh_min_length is not None and not 0 <= args.roh_min_length < 1 << 32:
            raise UsageError("--roh_min_length must be in [0, 2^32)")
        b = args.roh_bridge_sites
        if b is not None and b != 0 and not IBD_MIN_SITES <= b < 1 << 32:
            raise UsageError(f"--roh_bridge_sites must be 0 or at least {IBD_MIN_SITES} (and "
                             "below 2^32): shorter runs lie inside one 64-site word, which the "
                             "scan does not enumerate")
    if (args.mendel_trios or args.mendel_site_counts) and not args.mendel_uri:
        raise UsageError("--mendel_trios and --mendel_site_counts need --mendel_uri")
    if args.mendel_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--mendel_uri needs one process (one GPU): the trios are not "
                             "counted across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--mendel_uri needs --split_factor 1: it reads the samples of the "
                             "whole cohort's bitset")
        if not args.mendel_trios and not args.bed_uri:
            raise UsageError("--mendel_uri needs --mendel_trios: only the .fam under --bed_uri "
                             "declares parents")
    if (args.pihat_min is not None or args.pihat_unbounded) and not args.pihat_uri:
        raise UsageError("--pihat_min and --pihat_unbounded need --pihat_uri")
    if args.pihat_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--pihat_uri needs one process (one GPU): the scan is not split "
                             "across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--pihat_uri needs --split_factor 1: it scans the whole cohort's "
                             "pairs")
        if args.pihat_min is not None and args.pihat_min != args.pihat_min:
            raise UsageError("--pihat_min must not be NaN")
    if args.pcrelate_min_kinship is not None and not args.pcrelate_records_uri:
        raise UsageError("--pcrelate_min_kinship needs --pcrelate_records_uri")
    if args.pcrelate_records_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--pcrelate_records_uri needs one process (one GPU): the scan is "
                             "not split across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--pcrelate_records_uri needs --split_factor 1: it scans the whole "
                             "cohort's pairs")
        if not args.pca_uri:
            raise UsageError("--pcrelate_records_uri needs the principal components of the same "
                             "run: pass --pca_uri as well")
        t = args.pcrelate_min_kinship
        if t is not None and t != t:
            raise UsageError("--pcrelate_min_kinship must not be NaN")
    if args.pcrelate_uri:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise UsageError("--pcrelate_uri needs one process (one GPU): the matrix is not "
                             "assembled across ranks yet")
        if args.split_factor != 1:
            raise UsageError("--pcrelate_uri needs --split_factor 1: it writes the whole "
                             "cohort's matrix")
        if not args.pca_uri:
            raise UsageError("--pcrelate_uri needs the principal components of the same run: "
                             "pass --pca_uri as well")
    if args.pcrelate_uri or args.pcrelate_pairs_uri or args.pcrelate_records_uri:
        pca_k = 10 if args.pca_components is None else args.pca_components
        k = pcrelate_components(args)
        if k < 1 or k > pca_k:
            raise UsageError(f"--pcrelate_components must be between 1 and --pca_components "
                             f"({pca_k})")
        if k + 1 > PCRELATE_COLUMNS_MAX:
            raise UsageError(f"--pcrelate_components must be at most {PCRELATE_COLUMNS_MAX - 1} "
                             "(the intercept takes one of the kernel's "
                             f"{PCRELATE_COLUMNS_MAX} columns)")
        maf = args.pcrelate_min_maf
        if maf is not None and not 0.0 <= maf < 0.5:   # (false for a NaN)
            raise UsageError("--pcrelate_min_maf must be in [0, 0.5)")


PCRELATE_COLUMNS_MAX = 32   # (CUKING_PCRELATE_COLUMNS_MAX; host-only here: no library load)
IBD_MIN_SITES = 64          # (CUKING_IBD_MIN_SITES)


def pcrelate_components(args) -> int:
    """The number of components --pcrelate-uri adjusts for: its own flag, else all of the
    PCA's."""
    if args.pcrelate_components is not None:
        return args.pcrelate_components
    return 10 if args.pca_components is None else args.pca_components


def ld_pruning(args) -> bool:
    """Does the run prune by LD (any of its three flags)?"""
    return (args.site_ld_window is not None or args.site_ld_r2 is not None or
            bool(args.site_ld_uri))


def ld_rule(args):
    """--site-ld-window / --site-ld-r2 as the library sees them."""
    window = 50 if args.site_ld_window is None else args.site_ld_window
    r2 = 0.2 if args.site_ld_r2 is None else float(np.float32(args.site_ld_r2))
    if not 2 <= window <= 0xFFFFFFFF:
        raise UsageError("--site_ld_window must be at least 2 variants")
    if not 0.0 <= r2 <= 1.0:
        raise UsageError("--site_ld_r2 must be in [0, 1]")
    return window, r2


def site_filtering(args) -> bool:
    """Does the run drop sites (any of the five flags that select them)?"""
    return (args.site_min_call_rate is not None or args.site_min_maf is not None or
            args.site_min_mac is not None or args.site_hwe_p is not None or
            bool(args.site_keep_uri))


def hwe_rule(args):
    """--site-hwe-p / --site-hwe-midp as the library sees them: (threshold or None, midp)."""
    if args.site_hwe_p is None:
        if args.site_hwe_midp:
            raise UsageError("--site_hwe_midp needs --site_hwe_p")
        return None, False
    if not 0.0 <= args.site_hwe_p <= 1.0:   # (NaN fails)
        raise UsageError("--site_hwe_p must be in [0, 1]")
    return float(args.site_hwe_p), bool(args.site_hwe_midp)


def site_rule(args):
    """--site-min-call-rate / --site-min-maf / --site-min-mac as the library sees them."""
    rate = 0.0 if args.site_min_call_rate is None else float(np.float32(args.site_min_call_rate))
    maf = 0.0 if args.site_min_maf is None else float(np.float32(args.site_min_maf))
    mac = 0 if args.site_min_mac is None else args.site_min_mac
    if not 0.0 <= rate <= 1.0:
        raise UsageError("--site_min_call_rate must be in [0, 1]")
    if not 0.0 <= maf <= 1.0:
        raise UsageError("--site_min_maf must be in [0, 1]")
    if not 0 <= mac <= 0xFFFFFFFF:
        raise UsageError("--site_min_mac must be a count, 0 or more")
    return rate, maf, mac


def unrelated_threshold(args) -> float:
    """--unrelated-threshold as the library sees it (float32); --kin-threshold without it."""
    kin = float(np.float32(args.kin_threshold))
    if args.unrelated_threshold is None:
        return kin
    t = float(np.float32(args.unrelated_threshold))
    if t != t or t < kin:
        raise UsageError("--unrelated_threshold must not be below --kin_threshold (the records "
                         "hold no pair below it)")
    return t


def read_and_pack(in_dir: Path, sm, num_sites: int, threads: int) -> np.ndarray:
    """cuking.cu:529-711: list, decode, pack (host)."""
    import pyarrow.parquet as pq
    import cuking_amd
    files = sorted(p for p in in_dir.iterdir()
                   if p.is_file() and p.name.endswith(".parquet"))  # non-recursive
    if not files:
        raise RuntimeError("No input files found")
    bits = cuking_amd.new_host_bitset(sm, num_sites)

    def one(path):
        pf = pq.ParquetFile(path)
        if pf.metadata.num_columns != 3:
            raise RuntimeError(f"Expected 3 columns, found {pf.metadata.num_columns} in {path}")
        t = pf.read()
        cols = [t.column(k) for k in range(3)]  # by position (cuking.cu:585-597)
        if cols[0].null_count or cols[1].null_count:
            raise RuntimeError(f"null values are not allowed in row_idx/col_idx in {path}")
        alt = cols[2]
        if alt.null_count:  # null genotype = missing: drop the entry
            keep = alt.is_valid().to_numpy(zero_copy_only=False)
        else:
            keep = None
        row = cols[0].to_numpy().astype(np.int64, copy=False)
        col = cols[1].to_numpy().astype(np.int64, copy=False)
        a = alt.fill_null(0).to_numpy().astype(np.int32, copy=False)
        if keep is not None:
            row, col, a = row[keep], col[keep], a[keep]
        cuking_amd.pack_host(sm, bits, row, col, a)  # thread-safe atomics

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, files))
    return bits


def write_results(path: Path, recs: np.ndarray, sample_ids) -> None:
    """cuking.cu:767-863: REQUIRED columns, SNAPPY, one row group."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    ids = np.asarray(sample_ids, dtype=object)
    schema = pa.schema([pa.field("i", pa.string(), nullable=False),
                        pa.field("j", pa.string(), nullable=False),
                        pa.field("kin", pa.float32(), nullable=False),
                        pa.field("ibs0", pa.int32(), nullable=False),
                        pa.field("ibs1", pa.int32(), nullable=False),
                        pa.field("ibs2", pa.int32(), nullable=False)])
    table = pa.table({
        "i": pa.array(ids[recs["sample_i"]], pa.string()),
        "j": pa.array(ids[recs["sample_j"]], pa.string()),
        "kin": pa.array(recs["kin"], pa.float32()),
        "ibs0": pa.array(recs["ibs0"].astype(np.int32), pa.int32()),
        "ibs1": pa.array(recs["ibs1"].astype(np.int32), pa.int32()),
        "ibs2": pa.array(recs["ibs2"].astype(np.int32), pa.int32()),
    }, schema=schema)
    path.parent.mkdir(parents=True, exist_ok=True)
    pq.write_table(table, path, compression="snappy", use_dictionary=False,
                   row_group_size=max(len(recs), 1))


def write_kin_matrix(path: Path, ctx, sm, wps: int, bits, device: int) -> None:
    """The block's dense kinship matrix as a float32 .npy (a diagonal block symmetric)."""
    import torch
    rows, cols = sm.NumRows(), sm.NumCols()
    need = 4 * rows * cols
    free, _ = torch.cuda.mem_get_info(device)
    if need > free:
        raise RuntimeError(
            f"the kinship matrix of this block ({rows} x {cols} float32 = {need / 1e9:.1f} GB) "
            f"does not fit the {free / 1e9:.1f} GB free on the GPU: split the cohort into "
            "blocks with --split-factor (one matrix per shard)")
    kin = ctx.kin_matrix(sm, wps, bits, symmetric=sm.i_begin == sm.j_begin)
    torch.cuda.synchronize(device)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.save would append .npy to another suffix)
        np.save(f, kin.cpu().numpy())


def write_kin_summary(path: Path, ctx, sm, wps: int, bits, lo: float, hi: float, n: int) -> None:
    """The block's kinship summary as an .npz: the histogram and, per stored sample of the
    block (rows first, then columns), the nearest relative's kinship and global index."""
    summary = ctx.kin_summary(sm, wps, bits, lo=lo, hi=hi, bins=n)
    kin, partner = summary.nearest()
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, hist=summary.counts(), lo=np.float32(summary.lo), hi=np.float32(summary.hi),
                 bins=np.int64(n), best_kin=kin, best_partner=partner)


def write_relative_counts(path: Path, ctx, sm, wps: int, bits, thresholds, sample_ids) -> None:
    """The block's relative counts as an .npz: per stored sample of the block (rows first,
    then columns; `samples` names them) the partners in each band of `thresholds`."""
    counts = ctx.relative_counts(sm, wps, bits, thresholds=thresholds)
    stored = list(range(sm.i_begin, sm.i_end))
    if sm.i_begin != sm.j_begin:
        stored += list(range(sm.j_begin, sm.j_end))
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, bands=counts.bands(), thresholds=counts.thresholds,
                 samples=np.array([sample_ids[k] for k in stored], dtype=str))


def write_unrelated(path: Path, ctx, recs: np.ndarray, sample_ids, threshold: float,
                    priority_path, device: int) -> np.ndarray:
    """The unrelated set and the families of the records' graph as an .npz: per sample of the
    cohort (`samples` names them) `keep` (1 = stays) and `family` (the lowest index of its
    connected component), and the `threshold` above which a record was an edge.  Returns
    `keep`."""
    import torch
    n = len(sample_ids)
    priority = None
    if priority_path is not None:
        host = np.load(priority_path)
        if host.shape != (n,):
            raise ValueError(f"--unrelated_priority holds {host.shape}, the cohort has {n} samples")
        priority = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(
            f"cuda:{device}")
    words = np.ascontiguousarray(recs).view(np.int32).reshape(-1, 6)
    records = torch.from_numpy(words).to(f"cuda:{device}")
    got = ctx.unrelated_set(records, len(recs), n, threshold, priority=priority)
    path.parent.mkdir(parents=True, exist_ok=True)
    keep = got.keep.cpu().numpy()
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, keep=keep, family=got.family.cpu().numpy().view(np.uint32),
                 samples=np.array(list(sample_ids), dtype=str), threshold=np.float32(threshold))
    return keep


def write_pca(path: Path, ctx, bits, wps: int, num_sites: int, components: int, fit,
              sample_ids):
    """The principal components as an .npz: `eigenvalues` [k], `scores` [samples, k],
    `loadings` [sites, k], `allele_freq` and `sites_used` [sites] (of the sites QC and pruning
    left), `fit` [samples] (the samples the components were fitted on) and `samples`."""
    got = ctx.pca(bits, wps, num_sites, k=components, fit=fit)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, eigenvalues=got.eigenvalues, scores=got.scores, loadings=got.loadings,
                 allele_freq=got.allele_freq, sites_used=got.sites_used, fit=got.fit,
                 samples=np.array(list(sample_ids), dtype=str))
    return got


def write_pcrelate(path: Path, ctx, bits, wps: int, num_sites: int, pca, components: int,
                   min_maf: float, device: int) -> None:
    """The whole cohort's PC-Relate kinship matrix as a float32 .npy [samples, samples], from
    the leading `components` scores and the fit of this run's PCA."""
    import torch
    n = bits.shape[0]
    need = 4 * n * n
    free, _ = torch.cuda.mem_get_info(device)
    if need > free:
        raise RuntimeError(
            f"the PC-Relate matrix of this cohort ({n} x {n} float32 = {need / 1e9:.1f} GB) "
            f"does not fit the {free / 1e9:.1f} GB free on the GPU: call "
            "KingContext.pcrelate block by block instead (block=...)")
    scores = np.ascontiguousarray(pca.scores[:, :components])
    got = ctx.pcrelate(bits, wps, num_sites, scores, fit=pca.fit, min_maf=min_maf)
    torch.cuda.synchronize(device)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.save would append .npy to another suffix)
        np.save(f, got.kin.cpu().numpy())


def write_pcrelate_pairs(path: Path, ctx, bits, wps: int, num_sites: int, pca, components: int,
                         min_maf: float, recs, sample_ids) -> None:
    """This run's records re-scored by PC-Relate as an .npz: `sample_i`, `sample_j`, `kin`,
    `k0`, `k1`, `k2`, `ibs0`, `sites`, `relationship` (one entry per record, in the records'
    order; the codes of PCRelatePairs.relationship), `inbreeding` [samples] and `samples`."""
    scores = np.ascontiguousarray(pca.scores[:, :components])
    got = ctx.pcrelate_pairs(bits, wps, num_sites, recs, scores=scores, fit=pca.fit,
                             min_maf=min_maf)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample_i=got.sample_i, sample_j=got.sample_j, kin=got.kin, k0=got.k0,
                 k1=got.k1, k2=got.k2, ibs0=got.ibs0, sites=got.sites,
                 relationship=got.relationship(), inbreeding=got.inbreeding,
                 samples=np.array(list(sample_ids), dtype=str))


def write_pcrelate_records(path: Path, ctx, bits, wps: int, num_sites: int, pca, components: int,
                           min_maf: float, min_kinship: float, sample_ids) -> None:
    """The pairs of the whole cohort whose PC-Relate kinship is above `min_kinship` as an .npz:
    `sample_i`, `sample_j`, `kin` of the records sorted by (sample_i, sample_j); `k0`, `k1`,
    `k2`, `ibs0`, `sites`, `kin_pairs` (the pairs' own kinship) and `relationship` of
    pcrelate_pairs on them, in the same order; `samples`, `min_kinship`, `num_records`."""
    import torch
    scores = np.ascontiguousarray(pca.scores[:, :components])
    found = ctx.pcrelate_records(bits, wps, num_sites, scores=scores, fit=pca.fit,
                                 min_maf=min_maf, min_kinship=min_kinship)
    rows = found.sorted()
    dev = f"cuda:{ctx.device}"
    flat = torch.from_numpy(rows.view(np.int32).reshape(-1, 6).copy()).to(dev)
    got = ctx.pcrelate_pairs(bits, wps, num_sites, flat, model=found, min_maf=min_maf,
                             num_records=found.num_records)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample_i=rows["sample_i"], sample_j=rows["sample_j"], kin=rows["kin"],
                 k0=got.k0, k1=got.k1, k2=got.k2, ibs0=got.ibs0, sites=got.sites,
                 kin_pairs=got.kin, relationship=got.relationship(),
                 samples=np.array(list(sample_ids), dtype=str),
                 min_kinship=np.float32(found.min_kinship),
                 num_records=np.int64(found.num_records))


def write_pihat(path: Path, ctx, sm, bits, wps: int, num_sites: int, min_pi_hat: float,
                bounded: bool, sample_ids) -> None:
    """The pairs of the whole cohort whose PI_HAT is above `min_pi_hat` as an .npz: `sample_i`,
    `sample_j`, `pi_hat` (float32, the records' value), `z0`, `z1`, `z2` (float64), `ibs0`,
    `ibs1`, `ibs2` sorted by (sample_i, sample_j); `samples`; the model (`model`: e00, e01, e02,
    e11, e12; `sites_used`) of the cohort's own samples; `min_pi_hat`, `bounded`,
    `num_records`."""
    found = ctx.pi_hat_records(sm, wps, bits, num_sites, min_pi_hat, bounded=bounded)
    rows, z = found.sorted(), found.z()
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample_i=rows["sample_i"], sample_j=rows["sample_j"], pi_hat=rows["kin"],
                 z0=z[:, 0], z1=z[:, 1], z2=z[:, 2], ibs0=rows["ibs0"], ibs1=rows["ibs1"],
                 ibs2=rows["ibs2"], samples=np.array(list(sample_ids), dtype=str),
                 model=np.array(found.model.as_tuple()[:5], dtype=np.float64),
                 sites_used=np.int64(found.model.sites_used),
                 min_pi_hat=np.float32(found.min_pi_hat), bounded=np.bool_(found.bounded),
                 num_records=np.int64(found.num_records))


def write_ibd_segments(path: Path, ctx, bits, wps: int, num_sites: int, recs, group, pos,
                       site_index, min_sites: int, min_length: int, with_list: bool,
                       sample_ids, bridge_sites=None) -> None:
    """This run's records scanned for IBD segments as an .npz: `sample_i`, `sample_j`,
    `segments1`, `segments2`, `length1`, `length2`, `longest1`, `longest2`, `pi1`, `pi2`,
    `kin_ibd`, `relationship` (one entry per record, in the records' order; the codes of
    IBDPairs.relationship), `total_length`, `samples`, `min_sites`, `min_length`; with
    `with_list` the sorted segments as `segment_pair`, `segment_kind`, `segment_first_site`,
    `segment_last_site` (through `site_index`: numbers among the input's sites); with a
    `bridge_sites` (0 included) also `bridge_sites`, `bridged1` and `bridged2`."""
    got = ctx.ibd_segments(bits, wps, num_sites, recs, group=group, pos=pos,
                           min_sites=min_sites, min_length=min_length, segments=with_list,
                           bridge_sites=bridge_sites or 0)
    pi1, pi2, kin = got.proportions()
    extra = {}
    if bridge_sites is not None:
        bridged = got.bridged if got.bridged is not None else \
            np.zeros((len(got.rows), 2), dtype=np.uint32)   # (0: nothing is bridged)
        extra = dict(bridge_sites=np.int64(bridge_sites),
                     bridged1=np.ascontiguousarray(bridged[:, 0]),
                     bridged2=np.ascontiguousarray(bridged[:, 1]))
    if with_list:
        segs = got.sorted()
        extra.update(segment_pair=segs["pair"], segment_kind=segs["kind"],
                     segment_first_site=site_index[segs["first_site"]],
                     segment_last_site=site_index[segs["last_site"]])
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample_i=got.sample_i, sample_j=got.sample_j, segments1=got.segments1,
                 segments2=got.segments2, length1=got.length1, length2=got.length2,
                 longest1=got.longest1, longest2=got.longest2, pi1=pi1, pi2=pi2, kin_ibd=kin,
                 relationship=got.relationship(), total_length=np.int64(got.total_length),
                 samples=np.array(list(sample_ids), dtype=str), min_sites=np.int64(min_sites),
                 min_length=np.int64(min_length), **extra)


def write_ibd_scan(path: Path, ctx, bits, wps: int, num_sites: int, group, pos, min_sites: int,
                   min_length: int, min_total: int, sample_ids) -> None:
    """Every pair of this run scanned for IBD segments as an .npz: `sample_i`, `sample_j`,
    `segments1`, `segments2`, `length1`, `length2`, `longest1`, `longest2`, `pi1`, `pi2`,
    `kin_ibd`, `relationship` (one entry per pair with an IBD1 segment and `length1 >=
    min_total`, by (sample_i, sample_j); the codes of IBDPairs.relationship), `total_length`,
    `samples`, `min_sites`, `min_length`, `min_total`."""
    got = ctx.ibd_scan(bits, wps, num_sites, group=group, pos=pos, min_sites=min_sites,
                       min_length=min_length, min_total=min_total)
    pi1, pi2, kin = got.proportions()
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample_i=got.sample_i, sample_j=got.sample_j, segments1=got.segments1,
                 segments2=got.segments2, length1=got.length1, length2=got.length2,
                 longest1=got.longest1, longest2=got.longest2, pi1=pi1, pi2=pi2, kin_ibd=kin,
                 relationship=got.relationship(), total_length=np.int64(got.total_length),
                 samples=np.array(list(sample_ids), dtype=str), min_sites=np.int64(min_sites),
                 min_length=np.int64(min_length), min_total=np.uint64(min_total))


def write_roh(path: Path, ctx, bits, wps: int, num_sites: int, group, pos, site_index,
              min_sites: int, min_length: int, bridge_sites: int, with_list: bool,
              sample_ids) -> None:
    """Every sample of this run scanned for runs of homozygosity as an .npz: `sample`,
    `segments`, `length`, `longest`, `bridged`, `froh` (one entry per sample, in the cohort's
    order), `total_length`, `samples`, `min_sites`, `min_length`, `bridge_sites`; with
    `with_list` the sorted runs as `seg_sample`, `seg_first_site`, `seg_last_site` (through
    `site_index`: numbers among the input's sites)."""
    got = ctx.roh_segments(bits, wps, num_sites, group=group, pos=pos, min_sites=min_sites,
                           min_length=min_length, bridge_sites=bridge_sites, segments=with_list)
    extra = {}
    if with_list:
        segs = got.sorted()
        extra = dict(seg_sample=segs["pair"], seg_first_site=site_index[segs["first_site"]],
                     seg_last_site=site_index[segs["last_site"]])
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, sample=got.sample, segments=got.segments, length=got.length,
                 longest=got.longest, bridged=got.bridged, froh=got.froh(),
                 total_length=np.int64(got.total_length),
                 samples=np.array(list(sample_ids), dtype=str), min_sites=np.int64(min_sites),
                 min_length=np.int64(min_length), bridge_sites=np.int64(bridge_sites), **extra)


def load_mendel_trios(trios_path, bed_prefix, num_samples):
    """The trios of --mendel-uri as uint32 [T, 3] with NO_PARENT for an absent parent: the .npy of
    --mendel-trios, else what the .fam declares.  Host only; UsageError for what the user got
    wrong.  `num_samples`: the cohort's size where it is known by now, else None."""
    from cuking_amd import mendel, plink
    if trios_path is None:
        try:
            trios = mendel.trios_from_parents(plink.read_fam_parents(bed_prefix))
        except (OSError, ValueError) as e:
            raise UsageError(f"--mendel_uri: {e}") from e
        if len(trios) == 0:
            raise UsageError(f"--mendel_uri: {bed_prefix}.fam declares no parent that is in the "
                             "file: pass the trios with --mendel_trios")
        return trios
    try:
        listed = np.load(trios_path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise UsageError(f"--mendel_trios: cannot read {trios_path}: {e}") from e
    if listed.ndim != 2 or listed.shape[1] != 3 or listed.dtype.kind not in "iu":
        raise UsageError(f"--mendel_trios must hold an integer [T, 3] array, not {listed.dtype} "
                         f"{listed.shape}")
    listed = listed.astype(np.int64)
    limit = mendel.NO_PARENT if num_samples is None else num_samples
    if listed.size and (int(listed.min()) < -1 or int(listed.max()) >= limit or
                        int(listed[:, 0].min(initial=0)) < 0):
        raise UsageError("--mendel_trios must hold sample numbers below the cohort's size"
                         f"{'' if num_samples is None else f' ({num_samples})'}, -1 for an "
                         "absent parent only")
    return np.where(listed < 0, mendel.NO_PARENT, listed).astype(np.uint32)


def write_mendel(path: Path, ctx, bits, wps: int, num_sites: int, trios, with_sites: bool,
                 site_index, sample_ids) -> None:
    """The Mendelian errors of the listed trios as an .npz: `child`, `father`, `mother` (int64,
    -1 for an absent parent), `called`, `errors` [T, 8], `rate`, `per_sample` (one entry per
    sample of the cohort), `samples`; with `with_sites` also `site_errors` (one entry per site of
    the bitset) and `site_index` (those sites' numbers among the input's sites)."""
    from cuking_amd import mendel
    got = ctx.mendel_errors(bits, wps, num_sites, trios, site_counts=with_sites)
    extra = {}
    if with_sites:
        extra = dict(site_errors=got.site_errors, site_index=np.asarray(site_index))

    def number(who):
        return np.where(who == mendel.NO_PARENT, -1, who.astype(np.int64))
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:   # (np.savez would append .npz to another suffix)
        np.savez(f, child=number(got.child), father=number(got.father),
                 mother=number(got.mother), called=got.called, errors=got.errors,
                 rate=got.rate(), per_sample=got.per_sample(len(sample_ids)),
                 samples=np.array(list(sample_ids), dtype=str), **extra)


def site_qc(ctx, args, bits, wps: int, num_sites: int, sample_ids, keep_path, qc_path):
    """Site QC of the whole cohort's bitset: counts on the GPU, the rule on the host, the
    report if one is asked for, and -- with a flag that selects sites -- the compacted bitset.
    Returns (bits, words_per_sample, num_sites, kept_index) for everything behind: the kept
    sites' numbers among the input's."""
    import cuking_amd
    rate, maf, mac = site_rule(args)
    also = None
    if keep_path is not None:
        also = np.load(keep_path)
        if also.shape != (num_sites,):
            raise ValueError(f"--site_keep_uri holds {also.shape}, the cohort has {num_sites} "
                             "sites")
    min_hwe_p, hwe_midp = hwe_rule(args)
    d_counts = ctx.site_counts(bits, wps)
    extra = {}
    if min_hwe_p is not None:
        # the exact test on the device, from the counts where they lie; the rule on the host
        hwe_p = ctx.hwe_sites(d_counts, num_sites, midp=hwe_midp).cpu().numpy()
        also = cuking_amd.hwe_site_mask(hwe_p, min_hwe_p, also)
        extra = dict(hwe_p=hwe_p, min_hwe_p=np.float64(min_hwe_p), hwe_midp=np.bool_(hwe_midp))
    counts = d_counts.cpu().numpy().view(np.uint32)
    keep, kept = cuking_amd.site_mask_host(counts, num_sites, rate, maf, mac, also=also)
    if qc_path is not None:
        per_sample = ctx.sample_counts(bits, wps, num_sites).cpu().numpy().view(np.uint32)
        qc_path.parent.mkdir(parents=True, exist_ok=True)
        with open(qc_path, "wb") as f:   # (np.savez would append .npz to another suffix)
            np.savez(f, site_counts=counts[:num_sites],
                     keep=cuking_amd.site_mask_bool(keep, num_sites), sample_counts=per_sample,
                     samples=np.array(list(sample_ids), dtype=str),
                     min_call_rate=np.float32(rate), min_maf=np.float32(maf),
                     min_mac=np.uint32(mac), **extra)
    if not site_filtering(args):
        return bits, wps, num_sites, np.arange(num_sites)
    index = np.flatnonzero(cuking_amd.site_mask_bool(keep, num_sites))
    bits, wps, kept = ctx.compact_sites(bits, wps, keep, num_sites)
    print(f"[cuking_amd.run] site QC keeps {kept} of {num_sites} sites", flush=True)
    return bits, wps, kept, index


def ld_prune(ctx, args, bits, wps: int, num_sites: int, group, input_index, ld_path):
    """LD pruning of the bitset site QC left: edges and the kept set on the GPU, the report if
    one is asked for, the compacted bitset.  `group`: chromosome ids of the sites that enter,
    or None; `input_index`: their numbers among the input's sites.  Returns (bits,
    words_per_sample, num_sites, kept_index) for everything behind: the kept sites' numbers
    among the input's sites."""
    window, r2 = ld_rule(args)
    got = ctx.ld_prune(bits, wps, num_sites, window=window, r2=r2, group=group)
    kept_index = input_index[got.kept_index()]
    if ld_path is not None:
        ld_path.parent.mkdir(parents=True, exist_ok=True)
        with open(ld_path, "wb") as f:   # (np.savez would append .npz to another suffix)
            np.savez(f, keep=got.keep(), kept_index=kept_index,
                     num_edges=np.int64(got.num_edges), window=np.int64(window),
                     r2=np.float32(r2))
    print(f"[cuking_amd.run] LD pruning keeps {got.num_sites} of {num_sites} sites "
          f"({got.num_edges} edges)", flush=True)
    return got.bits, got.words_per_sample, got.num_sites, kept_index


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch
    import torch.distributed as dist
    import cuking_amd
    from cuking_amd.dist import GpuStagedOps, all_pairs_king_staged

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    try:
        validate(args)
        in_dir = resolve_uri(args.input_uri) if args.input_uri else None
        bed_prefix = resolve_uri(args.bed_uri) if args.bed_uri else None
        out_dir = resolve_uri(args.output_uri)
        kin_path = resolve_uri(args.kin_matrix_uri) if args.kin_matrix_uri else None
        summary_path = resolve_uri(args.kin_summary_uri) if args.kin_summary_uri else None
        counts_path = resolve_uri(args.relative_counts_uri) if args.relative_counts_uri else None
        unrelated_path = resolve_uri(args.unrelated_uri) if args.unrelated_uri else None
        priority_path = resolve_uri(args.unrelated_priority) if args.unrelated_priority else None
        site_keep_path = resolve_uri(args.site_keep_uri) if args.site_keep_uri else None
        site_qc_path = resolve_uri(args.site_qc_uri) if args.site_qc_uri else None
        site_ld_path = resolve_uri(args.site_ld_uri) if args.site_ld_uri else None
        pca_path = resolve_uri(args.pca_uri) if args.pca_uri else None
        pcrelate_path = resolve_uri(args.pcrelate_uri) if args.pcrelate_uri else None
        pairs_path = resolve_uri(args.pcrelate_pairs_uri) if args.pcrelate_pairs_uri else None
        records_path = resolve_uri(args.pcrelate_records_uri) if args.pcrelate_records_uri \
            else None
        ibd_path = resolve_uri(args.ibd_segments_uri) if args.ibd_segments_uri else None
        roh_path = resolve_uri(args.roh_uri) if args.roh_uri else None
        scan_path = resolve_uri(args.ibd_scan_uri) if args.ibd_scan_uri else None
        synthetic = None
        if args.synthetic:
            parts = [int(x) for x in args.synthetic.split(",")]
            if len(parts) not in (2, 3) or min(parts[:2]) <= 0:
                raise UsageError("--synthetic expects N,M[,seed]")
            synthetic = (parts[0], parts[1], parts[2] if len(parts) == 3 else 20240229)
        synth_model = 0
        if args.synthetic_model:  # (host-only: the names live in the library)
            names = cuking_amd.synth_models()
            if args.synthetic_model not in names:
                raise UsageError(f"Illegal value '{args.synthetic_model}' specified for flag "
                                 "'synthetic_model'")
            synth_model = names.index(args.synthetic_model)
        mendel_path = resolve_uri(args.mendel_uri) if args.mendel_uri else None
        mendel_trios = None
        if mendel_path is not None:   # (host only: a bad list is a usage error, before any GPU)
            known = synthetic[0] if synthetic else None
            if known is None and bed_prefix is not None:
                from cuking_amd import plink
                try:
                    known = len(plink.read_fam(bed_prefix))
                except (OSError, ValueError) as e:
                    raise UsageError(f"--mendel_uri: {e}") from e
            mendel_trios = load_mendel_trios(
                resolve_uri(args.mendel_trios) if args.mendel_trios else None, bed_prefix, known)
    except ValueError:
        if rank == 0:
            print("\nError: INVALID_ARGUMENT: --synthetic expects N,M[,seed]", file=sys.stderr)
        return 1
    except UsageError as e:
        if rank == 0:
            print(f"\nError: INVALID_ARGUMENT: {e}", file=sys.stderr)
        return 1
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", device_id=torch.device(dev))
    try:
        t0 = time.perf_counter()
        if synthetic:
            sample_ids = [f"S{k:07d}" for k in range(synthetic[0])]
            num_sites = synthetic[1]
        elif bed_prefix is not None:
            from cuking_amd import plink
            sample_ids, num_sites = plink.read_fam(bed_prefix), plink.count_sites(bed_prefix)
        else:
            meta = json.loads((in_dir / "metadata.json").read_text())
            sample_ids, num_sites = list(meta["samples"]), int(meta["num_sites"])
        sm = cuking_amd.Submatrix(len(sample_ids), args.split_factor, args.shard_index)
        wps = cuking_amd.words_per_sample(num_sites)
        ctx = cuking_amd.KingContext(local_rank)
        if args.variant >= 0:   # (every geometry call below goes through this context)
            ctx.set_option("variant", args.variant)
        stored = sm.NumSamples()
        bits = torch.zeros((max(stored, 1), wps), dtype=torch.int64, device=dev)
        # Rank 0 reads and packs; its outcome is agreed on before anybody
        # enters the data broadcast (a failed read must not hang the others).
        pack_error = None
        if rank == 0:
            try:
                if synthetic:
                    from cuking_amd.synth import cohort_to_device, plan_cohort
                    kind, pa, pb = cohort_to_device(plan_cohort(synthetic[0], synthetic[2]),
                                                    local_rank)
                    # the block's samples, rows first then columns (cuking.cu:171-175)
                    ctx.synth_bitset(synthetic[2], kind, pa, pb, sm.i_begin, sm.i_end,
                                     num_sites, out=bits[:sm.NumRows()], model=synth_model)
                    if sm.i_begin != sm.j_begin:
                        ctx.synth_bitset(synthetic[2], kind, pa, pb, sm.j_begin, sm.j_end,
                                         num_sites, out=bits[sm.NumRows():stored],
                                         model=synth_model)
                    torch.cuda.synchronize()
                elif bed_prefix is not None:
                    # dense 2-bit rows -> bitset on the device (csrc/king_bed.hip); a bad or
                    # truncated file raises here and is agreed on below like any read error
                    ctx.load_bed(bed_prefix, sm, out=bits)
                else:
                    host = read_and_pack(in_dir, sm, num_sites, args.num_reader_threads)
                    if stored:
                        bits[:stored].copy_(torch.from_numpy(host.view(np.int64)))
                print(f"[cuking_amd.run] packed {stored} samples x {num_sites} sites "
                      f"({time.perf_counter() - t0:.2f}s)", flush=True)
            except Exception as e:  # noqa: BLE001 - reported below on every rank
                pack_error = e
        if world > 1:
            ok = torch.tensor([0 if pack_error is None else 1], dtype=torch.int32, device=dev)
            dist.broadcast(ok, src=0)
            if int(ok) != 0 and pack_error is None:
                pack_error = RuntimeError("rank 0 failed to read the input")
        if pack_error is not None:
            raise RuntimeError(str(pack_error))
        if site_filtering(args) or site_qc_path is not None:
            # (one process, the whole cohort: validate) -- what follows sees the kept sites only
            bits, wps, num_sites, site_index = site_qc(ctx, args, bits[:stored], wps, num_sites,
                                                       sample_ids, site_keep_path, site_qc_path)
        else:
            site_index = np.arange(num_sites)
        if ld_pruning(args):
            # after the rule, on the bitset it left; chromosomes only a .bim names
            group = None
            if bed_prefix is not None:
                from cuking_amd import plink
                group = plink.read_bim_chromosomes(bed_prefix)[site_index]
            bits, wps, num_sites, site_index = ld_prune(ctx, args, bits[:stored], wps, num_sites,
                                                        group, site_index, site_ld_path)
        t1 = time.perf_counter()
        after_reserve = lambda: (0, 0)    # noqa: E731 - (allocations, host waits) since the reservation
        if sm.i_begin == sm.j_begin:
            # Diagonal block (the whole cohort when split_factor = 1): row bands
            # per rank, chunked broadcast overlapped with the kernel.
            local = cuking_amd.Submatrix.from_ranges(0, stored, 0, stored)
            ops = GpuStagedOps(ctx, local, wps, bits, args.kin_threshold, args.max_results)
            recs, _ = all_pairs_king_staged(ops, stored, ctx.tile_samples(), bits,
                                            num_chunks=args.chunks)
            after_reserve = ops.after_reserve
            if recs is not None:  # local -> global sample indices
                recs["sample_i"] += sm.i_begin
                recs["sample_j"] += sm.j_begin
        else:
            # Off-diagonal block: broadcast, then equal tile ranges per rank.
            from cuking_amd.dist import all_pairs_king
            results = torch.zeros((max(args.max_results, 1), 6), dtype=torch.int32, device=dev)
            index_flag = torch.zeros(2, dtype=torch.int32, device=dev)

            def compute_tiles(b, begin, end):
                index_flag.zero_()
                ctx.compute_king(sm, wps, b, args.kin_threshold, args.max_results, results,
                                 index_flag[0:1], index_flag[1:2], tile_range=(begin, end))
                count, ovf = (int(x) & 0xFFFFFFFF for x in index_flag.tolist())
                return results, min(count, args.max_results), int(ovf)

            if world > 1:
                # workspace before the first collective (cuking_ctx_reserve), as in the
                # staged pass
                ctx.reserve(sm, wps, [torch.cuda.current_stream()])
                at = (ctx.get_option("workspace_allocations"), ctx.get_option("host_syncs"))
                after_reserve = lambda: (ctx.get_option("workspace_allocations") - at[0],  # noqa: E731
                                         ctx.get_option("host_syncs") - at[1])
                recs, _ = all_pairs_king(compute_tiles, ctx.num_tiles(sm), bits)
            else:
                recs = ctx.run(sm, wps, bits, args.kin_threshold, args.max_results)
        # every rank's library-side allocations / host waits after its reservation
        # (must be 0: nothing blocks beside in-flight collectives)
        mine = torch.tensor(after_reserve(), dtype=torch.int64, device=dev)
        per_rank = [mine]
        if world > 1:
            per_rank = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(per_rank, mine)
        per_rank = [t.tolist() for t in per_rank]
        if rank == 0:
            dt = time.perf_counter() - t1
            out = out_dir / f"part-{args.shard_index:05d}.snappy.parquet"
            write_results(out, recs, sample_ids)
            if kin_path is not None:
                write_kin_matrix(kin_path, ctx, sm, wps, bits, local_rank)
            if summary_path is not None:
                write_kin_summary(summary_path, ctx, sm, wps, bits,
                                  *summary_bins(args.kin_summary_bins))
            if counts_path is not None:
                write_relative_counts(counts_path, ctx, sm, wps, bits,
                                      relative_thresholds(args.relative_thresholds), sample_ids)
            if args.pihat_uri:
                write_pihat(resolve_uri(args.pihat_uri), ctx, sm, bits, wps, num_sites,
                            cuking_amd.pihat.DEFAULT_MIN_PI_HAT if args.pihat_min is None
                            else args.pihat_min,
                            not args.pihat_unbounded, sample_ids)
            unrelated_keep = None
            if unrelated_path is not None:
                unrelated_keep = write_unrelated(unrelated_path, ctx, recs, sample_ids,
                                                 unrelated_threshold(args), priority_path,
                                                 local_rank)
            if pca_path is not None:
                fit = unrelated_keep == 1 if args.pca_fit == "unrelated" else None
                pca = write_pca(pca_path, ctx, bits[:stored], wps, num_sites,
                                10 if args.pca_components is None else args.pca_components, fit,
                                sample_ids)
                if pcrelate_path is not None:
                    write_pcrelate(pcrelate_path, ctx, bits[:stored], wps, num_sites, pca,
                                   pcrelate_components(args),
                                   0.01 if args.pcrelate_min_maf is None
                                   else args.pcrelate_min_maf, local_rank)
                if pairs_path is not None:
                    write_pcrelate_pairs(pairs_path, ctx, bits[:stored], wps, num_sites, pca,
                                         pcrelate_components(args),
                                         0.01 if args.pcrelate_min_maf is None
                                         else args.pcrelate_min_maf, recs, sample_ids)
                if records_path is not None:
                    write_pcrelate_records(records_path, ctx, bits[:stored], wps, num_sites, pca,
                                           pcrelate_components(args),
                                           0.01 if args.pcrelate_min_maf is None
                                           else args.pcrelate_min_maf,
                                           0.0442 if args.pcrelate_min_kinship is None
                                           else args.pcrelate_min_kinship, sample_ids)
            ibd_group = ibd_pos = None
            if (ibd_path is not None or roh_path is not None or scan_path is not None) and \
                    bed_prefix is not None:
                from cuking_amd import plink
                ibd_group = plink.read_bim_chromosomes(bed_prefix)[site_index]
                ibd_pos = plink.read_bim_positions(bed_prefix)[site_index]
            if roh_path is not None:
                write_roh(roh_path, ctx, bits[:stored], wps, num_sites, ibd_group, ibd_pos,
                          site_index, 512 if args.roh_min_sites is None else args.roh_min_sites,
                          0 if args.roh_min_length is None else args.roh_min_length,
                          args.roh_bridge_sites or 0, args.roh_segment_list, sample_ids)
            if mendel_path is not None:
                write_mendel(mendel_path, ctx, bits[:stored], wps, num_sites, mendel_trios,
                             args.mendel_site_counts, site_index, sample_ids)
            if ibd_path is not None:
                write_ibd_segments(ibd_path, ctx, bits[:stored], wps, num_sites, recs, ibd_group,
                                   ibd_pos, site_index,
                                   512 if args.ibd_min_sites is None else args.ibd_min_sites,
                                   0 if args.ibd_min_length is None else args.ibd_min_length,
                                   args.ibd_segment_list, sample_ids, args.ibd_bridge_sites)
            if scan_path is not None:
                write_ibd_scan(scan_path, ctx, bits[:stored], wps, num_sites, ibd_group, ibd_pos,
                               512 if args.ibd_scan_min_sites is None
                               else args.ibd_scan_min_sites,
                               0 if args.ibd_scan_min_length is None
                               else args.ibd_scan_min_length,
                               args.ibd_scan_min_total or 0, sample_ids)
            pairs = sm.NumPairs()
            print(json.dumps({"pairs": pairs, "results": int(len(recs)), "gpus": world,
                              "compute_seconds": dt,
                              "allocations_after_reserve": [int(x[0]) for x in per_rank],
                              "host_syncs_after_reserve": [int(x[1]) for x in per_rank],
                              "pairs_per_second": pairs / dt if dt > 0 else 0.0}), flush=True)
        rc = 0
    except cuking_amd.ResourceExhaustedError as e:
        if rank == 0:
            print(f"\nError: RESOURCE_EXHAUSTED: {e}", file=sys.stderr)
        rc = 1
    except (RuntimeError, cuking_amd.CukingError, OSError, KeyError, ValueError) as e:
        if rank == 0:
            print(f"\nError: FAILED_PRECONDITION: {e}", file=sys.stderr)
        rc = 1
    if world > 1 and dist.is_initialized():
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
