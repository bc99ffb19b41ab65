"""GPU box: the unrelated set on the device against the path a user had before it existed.

In ONE process, on the same device records, the two cases interleaved round by round (so
that clock drift and neighbours hit both alike), host clock around each whole call (both end
with the result on hand: the device call waits for its stream, the host path ends on the
host):

    d   KingContext.unrelated_set on the record buffer where compute_king left it
        (default priority, families on)
    h   copy the records to the host (24 B each), then cuking_unrelated_set_host

on the baseline synthetic cohort at BASELINE configs[1] (10k x 100k sites) and configs[2]
(100k x 100k) with the records of threshold 0.0442, and on one artificial buffer of 10^7
records: families planted as cliques of 56..80 samples over 300,000 samples, in shuffled
order.  The outputs of d and h must be equal, byte for byte.  Then the device call alone for
several round-batch sizes (env CUKING_AMD_PRUNE_BATCH: rounds enqueued between two reads of
the live count), which is what king_prune.hip's kRoundBatch was chosen from.

Reports median and range over the timed rounds and the expectation: d is not slower than h
at the 10^7-record buffer.

usage: python tools/unrelated_set_time.py [--rounds 10] [--warmup 2] [--out FILE] (appends)
                                          [--skip-c2]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

SEED = 20240229
THRESHOLD = 0.0442
BATCHES = (1, 2, 4, 8, 16, 32)


def cohort_records(ctx, n, m):
    """(device records [count, 6], count) of the baseline cohort at THRESHOLD."""
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    sm = cuking_amd.Submatrix(n)
    count = ctx.count_records(sm, bits.shape[1], bits, THRESHOLD)
    results = torch.zeros((max(count, 1), 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ctx.compute_king(sm, bits.shape[1], bits, THRESHOLD, count, results, index_flag[0:1],
                     index_flag[1:2])
    torch.cuda.synchronize()
    assert index_flag.tolist() == [count, 0]
    return results, count


def planted_records(num_samples=300_000, num_records=10_000_000, seed=7):
    """Cliques of 56..80 samples over a shuffled cohort, cut or repeated to num_records."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(num_samples).astype(np.int64)
    parts, at = [], 0
    while at + 80 <= num_samples:
        size = int(rng.integers(56, 81))
        a, b = np.triu_indices(size, 1)
        members = order[at:at + size]
        parts.append(np.stack([members[a], members[b]], axis=1))
        at += size
    pairs = np.concatenate(parts)
    pairs = np.resize(pairs[rng.permutation(len(pairs))], (num_records, 2))
    recs = np.zeros(num_records, dtype=cuking_amd.KING_RESULT_DTYPE)
    recs["sample_i"], recs["sample_j"] = pairs.min(axis=1), pairs.max(axis=1)
    recs["kin"] = rng.uniform(0.05, 0.5, size=num_records).astype(np.float32)
    words = torch.from_numpy(recs.view(np.int32).reshape(-1, 6))
    return words.to("cuda:0"), num_records


def measure(ctx, name, records, count, n, rounds, warmup, lines):
    def device():
        got = ctx.unrelated_set(records, count, n, THRESHOLD)
        return got.keep.cpu().numpy(), got.family.cpu().numpy().view(np.uint32), got.rounds

    def host():
        recs = records[:count].cpu().numpy()
        keep, family = cuking_amd.unrelated_set_host(recs, n, THRESHOLD)
        return keep, family, None

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return out, 1e3 * (time.perf_counter() - t0)

    times = {"d": [], "h": []}
    for rnd in range(warmup + rounds):
        (dk, df, dr), td = timed(device)
        (hk, hf, _), th = timed(host)
        assert dk.tobytes() == hk.tobytes() and df.tobytes() == hf.tobytes(), name
        if rnd >= warmup:
            times["d"].append(td)
            times["h"].append(th)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append(f"## {name}: {count} records, {n} samples, {int(dk.sum())} kept, "
                 f"{len(np.unique(df))} components, {dr} rounds; outputs equal")
    for k, what in (("d", "device unrelated_set"), ("h", "copy to host + host function")):
        t = times[k]
        lines.append(f"{k} {what:32s} median {med[k]:10.3f} ms  min {min(t):10.3f}  "
                     f"max {max(t):10.3f}")
    lines.append(f"ratio h / d {med['h'] / med['d']:.2f}")
    # the device call alone, per round-batch size
    per_batch = {}
    for batch in BATCHES:
        os.environ["CUKING_AMD_PRUNE_BATCH"] = str(batch)
        t = [timed(device)[1] for _ in range(warmup + rounds)][warmup:]
        per_batch[batch] = statistics.median(t)
        lines.append(f"d batch {batch:3d}: median {per_batch[batch]:10.3f} ms  min {min(t):10.3f}  "
                     f"max {max(t):10.3f}")
    del os.environ["CUKING_AMD_PRUNE_BATCH"]
    return {"records": count, "samples": n, "rounds": dr, "median_ms": med,
            "batch_median_ms": per_batch}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-c2", action="store_true")
    args = ap.parse_args(argv)
    if args.rounds < 10:
        ap.error("at least 10 timed rounds")
    ctx = cuking_amd.KingContext(0)
    lines = [f"# unrelated_set_time: threshold {THRESHOLD}, default priority, families on, "
             f"{args.warmup} warm-up + {args.rounds} timed rounds, cases interleaved, host clock "
             "ms per whole call",
             f"# device: {torch.cuda.get_device_name(0)}"]
    summary = {}
    cohorts = [("configs[1] 10k x 100k", 10_000, 100_000)]
    if not args.skip_c2:
        cohorts.append(("configs[2] 100k x 100k", 100_000, 100_000))
    for name, n, m in cohorts:
        records, count = cohort_records(ctx, n, m)
        summary[name] = measure(ctx, name, records, count, n, args.rounds, args.warmup, lines)
        del records
    records, count = planted_records()
    name = "planted 1e7 records / 300k samples"
    summary[name] = measure(ctx, name, records, count, 300_000, args.rounds, args.warmup, lines)
    med = summary[name]["median_ms"]
    lines.append(f"expectation d <= h at 1e7 records: {med['d']:.3f} <= {med['h']:.3f}: "
                 f"{'holds' if med['d'] <= med['h'] else 'DOES NOT HOLD'}")
    lines.append(json.dumps(summary))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
