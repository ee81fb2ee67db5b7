"""General encoder, one batch through every level: ms per call (device events, warm, median), GB/s of input and
total compressed bytes for levels 1, 2, 3 and RLE.

  python tools/leveltime.py [--n 8192] [--len 65536] [--reps 7] [--levels 1,2,3,rle]

FDH_LIB=<other libfdeflate_hip.so> times another build of the library on the same batch; FDH_GEN_LANES /
FDH_GEN_RESIDENT act as in the library."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd
from fdeflate_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--len", type=int, default=65536, dest="length")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--levels", default="1,2,3,rle")
ap.add_argument("--first", type=int, default=0, help="id of the first synthetic stream")
args = ap.parse_args()

assert torch.cuda.is_available(), "leveltime.py measures on a GPU"
MODES = {"1": fd.MODE_LEVEL1, "2": getattr(fd, "MODE_LEVEL2", 3), "3": getattr(fd, "MODE_LEVEL3", 4), "rle": fd.MODE_RLE}
n, L, dev = args.n, args.length, "cuda"
raw = synth.gen_batch_torch(args.first, n, L, device=dev)
bound = (fd.compress_bound(L) + 15) & ~15
in_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
c_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * bound
comp = torch.empty(n * bound, dtype=torch.uint8, device=dev)
clen = torch.empty(n, dtype=torch.int32, device=dev)
print("library %s; %d streams x %d bytes (synth from id %d)" % (fd._lib.SO_PATH, n, L, args.first))
for name in args.levels.split(","):
    mode = MODES[name]

    def step():
        return fd.deflate_general_batch(raw.view(-1), in_off, comp, c_off, mode, out_len=clen)

    step()      # warm: code objects, the workspace of this mode
    step()
    torch.cuda.synchronize()
    assert int((clen.view(torch.int32) == -1).sum()) == 0, "a slot was too small"
    total = int(clen.to(torch.int64).sum())
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print("level %-3s  %9.3f ms per call (median of %d, min %.3f, max %.3f)  %7.2f GB/s of input  %d compressed bytes (%.4f of input)"
          % (name, med, len(ms), min(ms), max(ms), n * L / med / 1e6, total, total / (n * L)))
