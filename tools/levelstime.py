"""Encoder levels 3, 4, 5, 6 and 9 on one batch, in one run: ms per call, GB/s of input and compressed size per level,
level 3 as the yardstick (tools/timing.py's method: device events, two warm-up calls, rounds in which the levels
alternate; median, minimum and maximum over the rounds).

  python tools/levelstime.py [--n 8192] [--len 65536] [--rounds 3] [--levels 3,4,5,6,9] [--out profiles/levels_time.txt]

The batch is the bench's: synth's PNG-filter-like streams (model D with rows).  synth has no text-like model, so there is
no second batch.  FDH_GEN_LANES / FDH_GEN_RESIDENT act as in the library."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import timing
import fdeflate_amd as fd
from fdeflate_amd import levels, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--len", type=int, default=65536, dest="length")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--levels", default="3,4,5,6,9")
ap.add_argument("--out", default=os.path.join("profiles", "levels_time.txt"))
args = ap.parse_args()

assert torch.cuda.is_available(), "levelstime.py measures on a GPU"
n, L = args.n, args.length
raw = synth.gen_batch_torch(0, n, L, device="cuda").view(-1)
bound = (fd.compress_bound(L) + 15) & ~15
in_off, c_off = timing.arange_off(n, L), timing.arange_off(n, bound)
comp = torch.empty(n * bound, dtype=torch.uint8, device="cuda")
clen = torch.empty(n, dtype=torch.int32, device="cuda")
todo = [int(x) for x in args.levels.split(",")]


def call(level):
    return lambda: levels.deflate_level_batch(raw, in_off, comp, c_off, level, out_len=clen)


sizes = {}
for level in todo:      # the sizes first: the timed rounds overwrite `clen`
    call(level)()
    torch.cuda.synchronize()
    assert int((clen == -1).sum()) == 0, "a slot was too small"
    sizes[level] = int(clen.to(torch.int64).sum())
ts, calls = timing.interleaved([("level %d" % level, call(level)) for level in todo], args.rounds, calls=1)
lines = ["%d streams x %d bytes of synth's PNG-filter-like data (%.1f MB), %s, %d CUs; per level: median [min .. max] over %d rounds of 1 call"
         % (n, L, n * L / 1e6, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, args.rounds),
         "plan of the lazy parser: lanes x wavefronts = %d x %d" % levels.level_plan(n, torch.cuda.get_device_properties(0).multi_processor_count, 6)]
base_ms = base_size = None
for level in todo:
    t = sorted(ts["level %d" % level])
    med = t[len(t) // 2]
    if base_ms is None:
        base_ms, base_size = med, sizes[level]
    lines.append("level %d  %10.3f ms [%10.3f .. %10.3f]  %8.3f GB/s of input  %11d compressed bytes (%.4f of input)  x%.2f the time and %+.2f %% the size of level %d"
                 % (level, med, t[0], t[-1], n * L / med / 1e6, sizes[level], sizes[level] / (n * L), med / base_ms,
                    100.0 * (sizes[level] - base_size) / base_size, todo[0]))
print("\n".join(lines))
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
