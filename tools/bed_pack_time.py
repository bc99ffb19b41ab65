#!/usr/bin/env python3
"""GPU box: what the PLINK .bed path costs against the triple path, on the same genotypes:

    bed_pack_time.py [samples] [sites] [files] [--no-parquet] [--random-bytes]
                                                (default 10000 x 100000 in 64 files)

  (a) cuking_pack_bed_device alone on rows resident on the GPU (HIP events, median of the
      repeats) and its bytes in + out per second
  (b) the host-to-device copy of the same bytes from pinned memory (HIP events, median)
  (c) KingContext.load_bed, wall time, the file in the page cache
  (d) the triple path on the same genotypes written as Parquet (the generator of
      tools/cli_timing.py): read+pack of `cuking --pack=device` and `--pack=host`, 16 reader
      threads -- the numbers of profiles/r04_pack_pipeline.txt re-measured on this box

--no-parquet leaves (d) out; --random-bytes fills the .bed with random bytes instead of
generating genotypes (every byte is legal; for sizes whose triples nobody wants to write:
100000 x 100000 is 2.5 GB as a .bed and 200 GB as triple columns), which implies it.
-> profiles/r07_bed_pack.txt
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def write_part(args):
    """The genotypes of tools/cli_timing.py write_part (same seed recipe), as one Parquet
    file of triples (unless `parquet` is false) and as .bed rows, which are returned."""
    out, f, lo, hi, n, seed, parquet = args
    from cuking_amd import plink
    rng = np.random.default_rng([seed, f])
    af = rng.uniform(0.05, 0.5, size=hi - lo)
    block = ((rng.random((hi - lo, n), dtype=np.float32) < af[:, None]).astype(np.int8) +
             (rng.random((hi - lo, n), dtype=np.float32) < af[:, None]).astype(np.int8))
    block[rng.random((hi - lo, n), dtype=np.float32) < 0.01] = -1
    block[:, n - 1] = block[:, 0]                 # one duplicate pair
    triples = int((block >= 0).sum())
    if parquet:
        import pyarrow as pa
        import pyarrow.parquet as pq
        row, col = np.nonzero(block >= 0)         # site-major, like the Spark writer
        table = pa.table({"row_idx": (row + lo).astype(np.int64),
                          "col_idx": col.astype(np.int64),
                          "n_alt_alleles": block[row, col].astype(np.int32)})
        pq.write_table(table, Path(out) / f"part-{f:05d}.zstd.parquet", compression="zstd",
                       compression_level=1, row_group_size=2_000_000)
    return triples, plink.encode_rows(block.T).tobytes()


def event_ms(fn, repeats, stream):
    """Median and minimum of `repeats` timings of fn() between two events on `stream`."""
    import torch
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        stop.record(stream)
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=10_000)
    ap.add_argument("m", type=int, nargs="?", default=100_000)
    ap.add_argument("files", type=int, nargs="?", default=64)
    ap.add_argument("--no-parquet", action="store_true")
    ap.add_argument("--random-bytes", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    parquet = not (a.no_parquet or a.random_bytes)
    import torch
    import cuking_amd
    from cuking_amd import plink
    if not torch.cuda.is_available():
        raise SystemExit("bed_pack_time.py measures on the GPU: no device found")
    n, m = a.n, a.m
    cpus = len(os.sched_getaffinity(0))
    threads = max(1, min(16, cpus))
    row_bytes = (n + 3) // 4
    d = Path(tempfile.mkdtemp(prefix="cuking_bedpack_"))
    try:
        (d / "in").mkdir()
        prefix = d / "cohort"
        ids = [f"S{k:07d}" for k in range(n)]
        t0 = time.perf_counter()
        Path(str(prefix) + ".fam").write_text("".join(f"{s} {s} 0 0 0 -9\n" for s in ids))
        Path(str(prefix) + ".bim").write_text("".join(f"1\tv{k}\t0\t{k + 1}\tA\tC\n"
                                                      for k in range(m)))
        triples = 0
        with open(str(prefix) + ".bed", "wb") as bed:
            bed.write(plink.MAGIC)
            if a.random_bytes:
                rng = np.random.default_rng(1)
                step = max(1, (256 << 20) // row_bytes)
                for lo in range(0, m, step):
                    bed.write(rng.bytes(min(step, m - lo) * row_bytes))
            else:
                (d / "in" / "metadata.json").write_text(json.dumps({"num_sites": m, "samples": ids}))
                bounds = np.linspace(0, m, a.files + 1).astype(int)
                jobs = [(str(d / "in"), f, int(bounds[f]), int(bounds[f + 1]), n, 1, parquet)
                        for f in range(a.files)]
                with ProcessPoolExecutor(threads) as ex:
                    for count, rows in ex.map(write_part, jobs):
                        triples += count
                        bed.write(rows)
        bed_bytes = os.path.getsize(str(prefix) + ".bed")
        pq_bytes = sum(p.stat().st_size for p in (d / "in").glob("*.parquet"))
        print(f"# {n} samples x {m} sites: .bed {bed_bytes / 1e6:.0f} MB (rows of {row_bytes} B)"
              + (f", {triples} triples" if triples else ", random bytes")
              + (f", {pq_bytes / 1e6:.0f} MB of zstd Parquet in {a.files} files" if parquet else "")
              + f"; written in {time.perf_counter() - t0:.1f} s; {cpus} hardware threads visible",
              flush=True)

        ctx = cuking_amd.KingContext(0)
        sm = cuking_amd.Submatrix(n)
        wps = cuking_amd.words_per_sample(m)
        out_bytes = n * wps * 8
        stream = torch.cuda.current_stream()
        with plink.open_bed(prefix) as bed:
            pinned = torch.empty(3 + m * row_bytes, dtype=torch.uint8).pin_memory()
            bed.read_rows(0, m, pinned.numpy()[3:])
        resident = torch.empty(3 + m * row_bytes, dtype=torch.uint8, device="cuda:0")
        rows = resident[3:]                       # misaligned, as in the file
        bits = torch.empty((n, wps), dtype=torch.int64, device="cuda:0")

        def copy():
            resident.copy_(pinned, non_blocking=True)

        def pack():
            ctx.pack_bed(sm, wps, rows, row_bytes, 0, m, m, bits)
        copy(), pack(), torch.cuda.synchronize()   # warm-up of both
        pack_med, pack_min = event_ms(pack, a.repeats, stream)
        copy_med, copy_min = event_ms(copy, a.repeats, stream)
        moved = m * row_bytes + out_bytes
        print(f"(a) pack_bed kernel, resident rows: median {pack_med:.3f} ms, min {pack_min:.3f} ms "
              f"of {a.repeats}; {m * row_bytes / 1e6:.0f} MB in + {out_bytes / 1e6:.0f} MB out = "
              f"{moved / pack_med / 1e6:.0f} GB/s", flush=True)
        print(f"(b) host-to-device copy of the rows (pinned): median {copy_med:.3f} ms, min "
              f"{copy_min:.3f} ms; {m * row_bytes / copy_med / 1e6:.1f} GB/s", flush=True)
        print(f"    (a) / (b) = {pack_med / copy_med:.3f}  (the pipeline runs at the speed of the "
              f"copy iff <= 1)", flush=True)
        one_shot = bits.clone()
        walls = []
        for _ in range(max(3, a.repeats // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loaded = ctx.load_bed(prefix, sm, out=bits)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        same = bool(torch.equal(loaded, one_shot))
        print(f"(c) load_bed (64 MiB chunks, page cache): wall median {statistics.median(walls):.3f} s, "
              f"min {min(walls):.3f} s of {len(walls)}; equals the one-shot pack: {same}", flush=True)
        if not same:
            raise SystemExit("load_bed differs from the one-shot pack")
        del pinned, resident, rows, bits, one_shot, loaded
        ctx.close()
        torch.cuda.empty_cache()
        if parquet:
            best = {}
            for rep in range(2):
                for pack_mode in ("device", "host"):
                    p = subprocess.run(["timeout", "-k", "10", "300", str(ROOT / "cuking_amd/bin/cuking"),
                                        "--input_uri", str(d / "in"), "--output_uri",
                                        str(d / f"out_{pack_mode}"), f"--pack={pack_mode}",
                                        "--decode=stream", f"--num_reader_threads={threads}",
                                        "--kin_threshold=0.05"], capture_output=True, text=True)
                    if p.returncode:
                        raise SystemExit(f"cuking --pack={pack_mode} failed ({p.returncode}): "
                                         f"{p.stderr[-800:]}")
                    s = json.loads(p.stdout.strip().splitlines()[-1])
                    best[pack_mode] = min(best.get(pack_mode, 1e30), s["read_pack_seconds"])
                    print(f"(d) rep {rep} cuking --pack={pack_mode:6s} --decode=stream: read+pack "
                          f"{s['read_pack_seconds']:.3f} s = {s['triples_per_second']:.3e} triples/s "
                          f"({threads} reader threads)", flush=True)
            better = min(best.values())
            print(f"# (c) min {min(walls):.3f} s against the better of (d) {better:.3f} s: "
                  f"{better / min(walls):.1f} x", flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
