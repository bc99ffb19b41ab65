"""GPU box: time of the synthetic generator for one bitset (default: BASELINE configs[2],
100,000 x 100,000), every cohort model through this tree's library -- and, with
PARENT_LIB=<path of a libcuking_amd.so built from another commit>, that library's
cuking_synth_bitset on the same device in the same process, for a before / after of the
baseline cohort.  Device events around the call, one warm-up call, median of five.

usage: [PARENT_LIB=path] python tools/synth_time.py [samples] [sites] [output file]
       the lines go to the console and, if one is named, to the output file
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import torch

import cuking_amd
from cuking_amd.synth import DEFAULT_SEED, cohort_to_device, plan_cohort

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None


def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


ctx = cuking_amd.KingContext(0)
cohort = plan_cohort(n, DEFAULT_SEED)
kind, pa, pb = cohort_to_device(cohort, 0)
wps = cuking_amd.words_per_sample(m)
bits = torch.empty((n, wps), dtype=torch.int64, device="cuda:0")



def timed(call):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)


say(f"# generator time, {n} samples x {m} sites ({bits.numel() * 8 / 1e9:.2f} GB bitset): device events "
    "around the call, after one warm-up call; median [min .. max] of five, ms")
keep = None
for k, name in enumerate(cuking_amd.synth_models()):
    ms = timed(lambda: ctx.synth_bitset(DEFAULT_SEED, kind, pa, pb, 0, n, m, out=bits, model=k))
    say(f"synth model {name}: {ms[2]:.2f} [{ms[0]:.2f} .. {ms[4]:.2f}]")
    if k == 0:
        keep = bits[:2000].cpu()

if not os.environ.get("PARENT_LIB"):
    sys.exit(0)
parent = C.CDLL(os.environ["PARENT_LIB"])
vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
parent.cuking_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
parent.cuking_synth_bitset.argtypes = [vp, u64, vp, vp, vp, u32, u32, u32, u32, vp, vp]
h = vp()
assert parent.cuking_ctx_create(0, C.byref(h)) == 0
stream = int(torch.cuda.current_stream().cuda_stream)


def parent_call():
    st = parent.cuking_synth_bitset(h, DEFAULT_SEED, kind.data_ptr(), pa.data_ptr(), pb.data_ptr(),
                                    0, n, m, wps, bits.data_ptr(), stream)
    assert st == 0


ms = timed(parent_call)
say(f"PARENT_LIB, cuking_synth_bitset: {ms[2]:.2f} [{ms[0]:.2f} .. {ms[4]:.2f}]")
say(f"first 2000 rows of the baseline equal the parent's: {bool(torch.equal(keep, bits[:2000].cpu()))}")
