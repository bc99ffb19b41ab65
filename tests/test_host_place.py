"""The host place runs without torch: every merged host entry point, called once in a fresh
process in which ``import torch`` fails, returns what it returns here with torch importable.
The host bodies share their code with the device's (cuking_amd/_place.py); the host twins run in
processes that never load torch."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# 3 samples x 128 sites (words_per_sample = 4), one pair / trio / block, min_sites = 64
COMPUTE = '''
import numpy as np
import cuking_amd
from cuking_amd import ibd, mendel, pcrelate, roh


def compute():
    rng = np.random.default_rng(11)
    n, m, wps = 3, 128, 4
    bits = np.zeros((n, wps), dtype=np.uint64)
    for s in range(n):       # a het every 16 sites or so, a hom-var now and then
        for site in range(m):
            u = rng.random()
            if u < 0.06:
                bits[s, site // 64] |= np.uint64(1) << np.uint64(site % 64)
            elif u < 0.07:
                bits[s, 2 + site // 64] |= np.uint64(1) << np.uint64(site % 64)
    x = np.ones((n, 1), dtype=np.float32)
    beta = np.full((m, 1), 0.3, dtype=np.float32)
    model = (bits, wps, m, x, beta, 0.01, 0.99)
    table = rng.standard_normal((m, 4)).astype(np.float32)
    rhs = rng.standard_normal((m, 1)).astype(np.float32)
    site_bits = cuking_amd.transpose_sites_host(bits, wps, m)
    got = {}
    r = ibd.ibd_segments_host(bits, wps, m, [[0, 1]], min_sites=64, segments=True)
    got["ibd_segments_host"] = [r.rows, r.sorted(), r.total_length]
    r = ibd.ibd_scan_host(bits, wps, m, min_sites=64)
    got["ibd_scan_host"] = [r.rows, r.total_length, r.block.as_tuple()]
    r = roh.roh_segments_host(bits, wps, m, [2], min_sites=64, segments=True)
    got["roh_segments_host"] = [r.rows, r.sorted(), r.total_length]
    r = mendel.mendel_errors_host(bits, wps, m, [[0, 1, 2]], site_counts=True)
    got["mendel_errors_host"] = [r.rows, r.site_errors]
    got["pcrelate_matrix_host"] = [pcrelate.pcrelate_matrix_host(*model)]
    got["pcrelate_pairs_raw_host"] = [pcrelate.pcrelate_pairs_raw_host(*model, [[0, 1]])]
    got["pcrelate_records_raw_host"] = list(
        pcrelate.pcrelate_records_raw_host(*model, float("-inf")))
    got["ld_edges_host"] = list(cuking_amd.ld_edges_host(site_bits, m, n, window=50, r2=0.0))
    got["geno_matmul_host"] = [cuking_amd.geno_matmul_host(bits, wps, m, table, rhs)]
    return {name: [[str(v.dtype), list(v.shape), v.tobytes().hex()]
                   if isinstance(v, np.ndarray) else v for v in values]
            for name, values in got.items()}
'''

CHILD = '''
import json, sys
sys.modules["torch"] = None     # import torch raises ImportError from here on
sys.path.insert(0, sys.argv[1])
''' + COMPUTE + '''
print(json.dumps(compute()))
assert sys.modules["torch"] is None
'''


def test_host_entry_points_run_without_torch_and_agree():
    here = {}
    exec(COMPUTE, here)
    want = json.loads(json.dumps(here["compute"]()))
    # the inputs reach the library with work to do
    assert want["ibd_segments_host"][0][1] == [1] and want["ibd_scan_host"][0][1][0] >= 1
    assert want["pcrelate_records_raw_host"][1] == 3 and want["ld_edges_host"][1] >= 1
    assert want["mendel_errors_host"][1][1] == [128] and want["roh_segments_host"][0][1] == [1]
    child = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], capture_output=True,
                           text=True)
    assert child.returncode == 0, child.stderr
    got = json.loads(child.stdout.splitlines()[-1])
    assert sorted(got) == sorted(want) and len(got) == 9
    for name in want:
        assert got[name] == want[name], name
