"""Times PNG encode at a compression level (fdeflate_amd.png_levels) at the bench shape (n x (341 x 64) RGB8 pictures),
and writes what it prints to profiles/png_levels_time.txt as well.

    python tools/pnglevelstime.py [--n 65536] [--pipeline-n 8192] [--rounds 5] [--out profiles/png_levels_time.txt]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE (tools/timing.py); per
variant: median [minimum .. maximum] over the rounds.  The pictures are the bench's synthetic RGB8 rows.
  (1) png_filter_mixed_batch in chosen mode on n pictures against the two-call route that gives the same bytes:
      png_choose_filters_mixed_batch, then png_filter_batch with its types; and in given mode against png_filter_batch
      alone.  Traffic: the fused kernel's bytes (pixels once, filtered rows and types once) per pixel byte, against the
      route's (pixels twice, types twice, filtered rows once).
  (2) png_encode_mixed_rgba_files_level_batch on pipeline-n pictures at levels 1, 3 and 6, end to end, against
      levels.deflate_level_batch alone on the same filtered bytes: the difference is what the PNG layer adds.  File sizes
      against the ultra-fast pipeline's (png_encode_mixed_rgba_files_batch) on the same pictures.
"""
import argparse
import builtins
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import levels, png_levels, synth  # noqa: E402
import timing  # noqa: E402
from timing import arange_off  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--pipeline-n", type=int, default=8192)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join("profiles", "png_levels_time.txt"))
args = ap.parse_args()
dev = "cuda"
log = open(args.out, "w")


def print(*a, **k):  # noqa: A001 (everything the tool and tools/timing.py print goes to the file as well)
    builtins_print(*a, **k)
    builtins_print(*a, **dict(k, file=log))
    log.flush()


builtins_print = builtins.print
timing.print = print

# ---- the bench's synthetic PNG rows as packed RGB8 scanlines and as RGBA8 pictures ----
n, L = args.n, 65536
width, rows = (synth.ROW_BYTES - 1) // 3, L // synth.ROW_BYTES
rb, bpp = fd.png_geometry(width, 8, 2)
filtered = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
pix = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
p_off, t_off, f_off = arange_off(n, rows * rb), arange_off(n, rows), arange_off(n, rows * (rb + 1))
fd.png_unfilter_batch(filtered, arange_off(n, L), pix, p_off, rb, bpp)
del filtered
info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
info[:, 1], info[:, 2], info[:, 3] = width, rows, 8 | 2 << 8
print("%d x (%d x %d) RGB8: %d bytes of packed scanlines and %d of filtered rows each" % (n, width, rows, rows * rb, rows * (rb + 1)))

# ---- (1) the kernel ----
types_a, types_b = torch.empty(n * rows, dtype=torch.uint8, device=dev), torch.empty(n * rows, dtype=torch.uint8, device=dev)
filt_a, filt_b = torch.empty(n * rows * (rb + 1), dtype=torch.uint8, device=dev), torch.empty(n * rows * (rb + 1), dtype=torch.uint8, device=dev)
st_a, st_b, st_c = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
fused = lambda: png_levels.png_filter_mixed_batch(pix, p_off, types_a, t_off, filt_a, f_off, info, png_status=st_a)
choose = lambda: fd.png_choose_filters_mixed_batch(pix, p_off, types_b, t_off, info, png_status=st_b)
filt = lambda: fd.png_filter_batch(pix, p_off, types_b, t_off, filt_b, f_off, rb, bpp, png_status=st_c)
given = lambda: png_levels.png_filter_mixed_batch(pix, p_off, types_b, t_off, filt_a, f_off, info, flags=png_levels.PNG_FILTER_GIVEN_TYPES,
                                                  png_status=st_a)


def route():
    choose()
    filt()


fused(), route()
torch.cuda.synchronize()
print("(1) types and filtered rows of the fused kernel are the route's: %s; statuses all 0: %s" %
      (torch.equal(types_a, types_b) and torch.equal(filt_a, filt_b), int(st_a.abs().sum() + st_b.abs().sum() + st_c.abs().sum()) == 0))
stats = timing.measure((("png_filter_mixed_batch, chosen (one pass)", fused), ("png_choose_filters_mixed_batch + png_filter_batch", route),
                        ("  png_choose_filters_mixed_batch alone", choose), ("  png_filter_batch alone", filt),
                        ("png_filter_mixed_batch, given types", given)), args.rounds)
(m, mlo, mhi), (p, plo, phi) = stats[0], stats[1]
spread = max(mhi - mlo, phi - plo)
print("  fused / route = %.3f (%+.3f ms); the larger min-max spread of the two %.3f ms: the fused kernel is %s" %
      (m / p, m - p, spread, "faster by more than the spread" if p - m > spread else "NOT faster by more than the spread"))
pixel_bytes = n * rows * rb
fused_bytes, route_bytes = pixel_bytes + n * rows * (rb + 1) + n * rows, 2 * pixel_bytes + n * rows * (rb + 1) + 2 * n * rows
print("  traffic per pixel byte: fused %.3f (1 x read + 1 x write; %.3f TB/s), the route %.3f (2 x read + 1 x write; %.3f TB/s)" %
      (fused_bytes / pixel_bytes, fused_bytes / m / 1e9, route_bytes / pixel_bytes, route_bytes / p / 1e9))
print("  given types: mixed kernel / png_filter_batch = %.3f" % (stats[4][0] / stats[3][0]))
del types_a, types_b, filt_b, st_b, st_c

# ---- (2) the pipeline ----
n2 = min(args.pipeline_n, n)
pix2, info2 = pix[:n2 * rows * rb], info[:n2]
rgba = torch.empty(n2 * rows * width * 4, dtype=torch.uint8, device=dev)
r_off = arange_off(n2, rows * width * 4)
assert int(fd.png_expand_batch(pix2, p_off[:n2 + 1], rgba, r_off, width, 8, 2).abs().sum()) == 0
w_t = torch.full((n2,), width, dtype=torch.int32, device=dev)
h_t = torch.full((n2,), rows, dtype=torch.int32, device=dev)
filt2, f_off2 = filt_a[:n2 * rows * (rb + 1)], f_off[:n2 + 1]
fast = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, w_t, h_t, pairs=(8, 2))
torch.cuda.synchronize()
fast_bytes = int(fast[2].to(torch.int64).sum())
print("(2) %d pictures; the ultra-fast pipeline's files: %.1f bytes each (statuses all 0: %s)" % (n2, fast_bytes / n2, int(fast[3].abs().sum()) == 0))
del fast
timing.measure((("png_encode_mixed_rgba_files_batch (ultra-fast)", lambda: fd.png_encode_mixed_rgba_files_batch(rgba, r_off, w_t, h_t, pairs=(8, 2))),),
               args.rounds)
for level in (1, 3, 6):
    slot = (png_levels.level_bound(rows * (rb + 1), level) + 15) & ~15
    out, o_off, o_len = torch.empty(n2 * slot, dtype=torch.uint8, device=dev), arange_off(n2, slot), torch.empty(n2, dtype=torch.int32, device=dev)
    res = png_levels.png_encode_mixed_rgba_files_level_batch(rgba, r_off, w_t, h_t, level, pairs=(8, 2))
    levels.deflate_level_batch(filt2, f_off2, out, o_off, level, out_len=o_len)
    torch.cuda.synchronize()
    size = int(res[2].to(torch.int64).sum())
    print("    level %d: files %.1f bytes each, %.3f of the ultra-fast pipeline's (%s); statuses all 0: %s; the streams are deflate_level_batch's + 57 bytes: %s" %
          (level, size / n2, size / fast_bytes, "smaller" if size < fast_bytes else "LARGER", int(res[3].abs().sum()) == 0,
           torch.equal(res[2], o_len + 57)))
    del res
    stats = timing.measure((("png_encode_mixed_rgba_files_level_batch, level %d" % level,
                             lambda: png_levels.png_encode_mixed_rgba_files_level_batch(rgba, r_off, w_t, h_t, level, pairs=(8, 2))),
                            ("levels.deflate_level_batch alone, level %d" % level,
                             lambda: levels.deflate_level_batch(filt2, f_off2, out, o_off, level, out_len=o_len))), args.rounds)
    print("    level %d: the PNG layer adds %.3f ms to the encoder's %.3f ms (pipeline / encoder = %.3f)" %
          (level, stats[0][0] - stats[1][0], stats[1][0], stats[0][0] / stats[1][0]))
    del out
log.close()
