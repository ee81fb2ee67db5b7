"""Times the RGBA16 mixed encode (fdeflate_amd.png16_encode) against its nearest existing relatives, at the bench shape
(n x (341 x 64) pictures), and writes what it prints to profiles/png16_encode_time.txt as well.

    python tools/png16enctime.py [--n 65536] [--rounds 5] [--out profiles/png16_encode_time.txt]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE (tools/timing.py); per
variant: median [minimum .. maximum] over the rounds.  The pictures are the bench's synthetic RGB8 rows: NARROW ones are
those samples * 257 (both bytes equal), WIDE ones have the same high bytes and noise in the low bytes of R, G and B (A
stays 65535), so that the plan gives them (16, 2).
  (1) png_analyse16_mixed_batch on the narrow pictures against png_analyse_mixed_batch on their high bytes
  (2) png_pack16_mixed_batch at (16, 2) on the wide pictures against png16.png_pack16_batch: the same body
  (3) png_pack16_mixed_batch at (8, 2) on the narrow pictures against png_pack_mixed_batch on the high bytes
  (4) png_encode_mixed_rgba16_files_batch on the narrow pictures against png_encode_mixed_rgba_files_batch on the high bytes
  (5) png_encode_mixed_rgba16_files_batch on the wide pictures against png16.png_encode_rgba16_files_batch at (16, 2)
"""
import argparse
import builtins
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import png16, png16_encode, synth  # noqa: E402
import timing  # noqa: E402
from timing import arange_off  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join("profiles", "png16_encode_time.txt"))
args = ap.parse_args()
dev = "cuda"
log = open(args.out, "w")


def print(*a, **k):  # noqa: A001 (everything the tool and tools/timing.py print goes to the file as well)
    builtins_print(*a, **k)
    builtins_print(*a, **dict(k, file=log))
    log.flush()


builtins_print = builtins.print
timing.print = print


def compare(title, variants, read_bytes=None):
    """The first variant is the RGBA16 call, the second its relative: ratio, difference, and the relative's own spread."""
    stats = timing.measure(variants, args.rounds, width=66)
    (m, _, _), (p, plo, phi) = stats[0], stats[1]
    print("  %s: RGBA16 call / relative = %.3f (%+.3f ms); the relative's spread over the rounds %.3f ms: %s" %
          (title, m / p, m - p, phi - plo, "inside" if abs(m - p) <= phi - plo else "outside, faster" if m < p else "outside, slower"))
    if read_bytes:
        print("  %s: reads %.3f TB/s (%.2f GB) against %.3f TB/s (%.2f GB)" %
              (title, read_bytes[0] / m / 1e9, read_bytes[0] / 1e9, read_bytes[1] / p / 1e9, read_bytes[1] / 1e9))
    sys.stdout.flush()
    return stats


def records(n, width, height, depth, colour):
    info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    info[:, 1], info[:, 2], info[:, 3] = width, height, depth | colour << 8
    return info


# ---- the bench's synthetic PNG rows as RGBA8, narrow RGBA16 and wide RGBA16 pictures ----
n, L = args.n, 65536
width, rows = (synth.ROW_BYTES - 1) // 3, L // synth.ROW_BYTES
rb8, bpp8 = fd.png_geometry(width, 8, 2)
rb16, bpp16 = fd.png_geometry(width, 16, 2)
filtered = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
pixels = torch.empty(n * rows * rb8, dtype=torch.uint8, device=dev)
fd.png_unfilter_batch(filtered, arange_off(n, L), pixels, arange_off(n, rows * rb8), rb8, bpp8)
del filtered
rgba8 = torch.empty(n * rows * width * 4, dtype=torch.uint8, device=dev)
off8, off16 = arange_off(n, rows * width * 4), arange_off(n, rows * width * 8)
assert int(fd.png_expand_batch(pixels, arange_off(n, rows * rb8), rgba8, off8, width, 8, 2).abs().sum()) == 0
del pixels
narrow = torch.stack((rgba8, rgba8), dim=1).view(-1)                       # low byte, high byte: s * 257
g = torch.Generator(device=dev)
g.manual_seed(16)
low = torch.randint(0, 256, (n * rows * width, 4), generator=g, device=dev, dtype=torch.uint8)
low[:, 3] = 255
wide = torch.stack((low.view(-1), rgba8), dim=1).view(-1)
del low
w_t = torch.full((n,), width, dtype=torch.int32, device=dev)
h_t = torch.full((n,), rows, dtype=torch.int32, device=dev)
dims = fd.png_encode_records(w_t, h_t)
print("%d x (%d x %d): %d bytes of RGBA16 and %d of RGBA8 each; %d bytes packed at (16, 2), %d at (8, 2)" %
      (n, width, rows, rows * width * 8, rows * width * 4, rows * rb16, rows * rb8))

# ---- (1) analysis ----
out = [torch.empty((n, 256), dtype=torch.int32, device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev),
       torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
out2 = [torch.empty_like(t) for t in out]
analyse16 = lambda: png16_encode.png_analyse16_mixed_batch(narrow, off16, dims, pal=out[0], colour=out[1], trns_len=out[2], summary=out[3],
                                                           png_status=out[4])
analyse8 = lambda: fd.png_analyse_mixed_batch(rgba8, off8, dims, pal=out2[0], colour=out2[1], trns_len=out2[2], summary=out2[3], png_status=out2[4])
analyse16(), analyse8()
torch.cuda.synchronize()
print("(1) analysis of the narrow pictures; the outputs are the RGBA8 analysis' (summary | 4): %s; statuses %s" %
      (all(torch.equal(a, b) for a, b in zip(out[:3] + out[4:], out2[:3] + out2[4:])) and torch.equal(out[3], out2[3] | 4),
       sorted(set(out[4].unique().tolist()))))
compare("(1) analyse", (("png_analyse16_mixed_batch (narrow RGBA16)", analyse16), ("png_analyse_mixed_batch (their high bytes)", analyse8)),
        (narrow.numel(), rgba8.numel()))
png16_encode.png_analyse16_mixed_batch(wide, off16, dims, pal=out[0], colour=out[1], trns_len=out[2], summary=out[3], png_status=out[4])
torch.cuda.synchronize()
print("    the wide pictures: statuses %s, summaries %s" % (sorted(set(out[4].unique().tolist())), [hex(v) for v in out[3].unique().tolist()]))
timing.measure((("png_analyse16_mixed_batch (wide RGBA16: insertion stops)",
                 lambda: png16_encode.png_analyse16_mixed_batch(wide, off16, dims, pal=out[0], colour=out[1], trns_len=out[2], summary=out[3],
                                                                png_status=out[4])),), args.rounds, width=66)
del out, out2

# ---- (2) packing at (16, 2) ----
st, st2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
info16 = records(n, width, rows, 16, 2)
p_off16 = arange_off(n, rows * rb16)
pix_a, pix_b = torch.empty(n * rows * rb16, dtype=torch.uint8, device=dev), torch.empty(n * rows * rb16, dtype=torch.uint8, device=dev)
pack_mixed16 = lambda: png16_encode.png_pack16_mixed_batch(wide, off16, pix_a, p_off16, info16, png_status=st)
pack_one16 = lambda: png16.png_pack16_batch(wide, off16, pix_b, p_off16, width, 2, png_status=st2)
pack_mixed16(), pack_one16()
torch.cuda.synchronize()
print("(2) packing at (16, 2); the two calls agree: %s" % (int(st.abs().sum()) == 0 and int(st2.abs().sum()) == 0 and torch.equal(pix_a, pix_b)))
compare("(2) pack (16, 2)", (("png_pack16_mixed_batch (16, 2)", pack_mixed16), ("png16.png_pack16_batch (per geometry)", pack_one16)))
del pix_a, pix_b

# ---- (3) packing at (8, 2) ----
info8 = records(n, width, rows, 8, 2)
p_off8 = arange_off(n, rows * rb8)
pix_a, pix_b = torch.empty(n * rows * rb8, dtype=torch.uint8, device=dev), torch.empty(n * rows * rb8, dtype=torch.uint8, device=dev)
pack_mixed8 = lambda: png16_encode.png_pack16_mixed_batch(narrow, off16, pix_a, p_off8, info8, png_status=st)
pack_one8 = lambda: fd.png_pack_mixed_batch(rgba8, off8, pix_b, p_off8, info8, png_status=st2)
pack_mixed8(), pack_one8()
torch.cuda.synchronize()
print("(3) packing at (8, 2); the two calls agree: %s" % (int(st.abs().sum()) == 0 and int(st2.abs().sum()) == 0 and torch.equal(pix_a, pix_b)))
compare("(3) pack (8, 2)", (("png_pack16_mixed_batch (8, 2) (narrow RGBA16)", pack_mixed8), ("png_pack_mixed_batch (8, 2) (their high bytes)", pack_one8)),
        (narrow.numel(), rgba8.numel()))
del pix_a, pix_b

# ---- (4) the pipeline on narrow pictures ----
def same_files(a, b):
    """Offsets, lengths and statuses equal, and every byte inside a file equal (the slots are larger than the files, and
    what lies behind a file is not specified)."""
    if not (torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])):
        return False
    if torch.equal(a[0], b[0]):
        return True
    edge = torch.zeros(a[0].numel() + 1, dtype=torch.int32, device=dev)
    start = a[1][:-1]
    one = torch.ones(start.numel(), dtype=torch.int32, device=dev)
    edge.index_add_(0, start, one)
    edge.index_add_(0, start + a[2].to(torch.int64), -one)
    inside = torch.cumsum(edge[:-1], 0, dtype=torch.int32) > 0
    return bool(((a[0] == b[0]) | ~inside).all())


a = png16_encode.png_encode_mixed_rgba16_files_batch(narrow, off16, w_t, h_t)
b = fd.png_encode_mixed_rgba_files_batch(rgba8, off8, w_t, h_t)
torch.cuda.synchronize()
print("(4) the pipeline on the narrow pictures: %d files, (depth | colour << 8) %s; byte-identical to the RGBA8 pipeline's: %s; %.3f GB of files" %
      (int((a[3] == 0).sum()), sorted(set((a[4][:, 3] & 0xFFFF).unique().tolist())), same_files(a, b), int(a[2].to(torch.int64).sum()) / 1e9))
del a, b
compare("(4) pipeline, narrow", (("png_encode_mixed_rgba16_files_batch (narrow RGBA16)", lambda: png16_encode.png_encode_mixed_rgba16_files_batch(narrow, off16, w_t, h_t)),
                                 ("png_encode_mixed_rgba_files_batch (their high bytes)", lambda: fd.png_encode_mixed_rgba_files_batch(rgba8, off8, w_t, h_t))))

# ---- (5) the pipeline on wide pictures ----
slot = (fd.png_file_bound(rows, rb16) + 15) & ~15
f_off = arange_off(n, slot)
files = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
a = png16_encode.png_encode_mixed_rgba16_files_batch(wide, off16, w_t, h_t)
f_len, f_st = png16.png_encode_rgba16_files_batch(wide, off16, files, f_off, width, 2)
back = png16.png_decode_mixed_files_rgba16_batch(a[0], a[1], file_len=a[2])
torch.cuda.synchronize()
print("(5) the pipeline on the wide pictures: %d files, (depth | colour << 8) %s; the lengths are the depth-16 pipeline's: %s; decoded back to the input: %s; %.3f GB of files" %
      (int((a[3] == 0).sum()), sorted(set((a[4][:, 3] & 0xFFFF).unique().tolist())), int(f_st.abs().sum()) == 0 and torch.equal(a[2], f_len),
       torch.equal(back[0], wide), int(a[2].to(torch.int64).sum()) / 1e9))
del a, back
compare("(5) pipeline, wide", (("png_encode_mixed_rgba16_files_batch (wide RGBA16)", lambda: png16_encode.png_encode_mixed_rgba16_files_batch(wide, off16, w_t, h_t)),
                               ("png16.png_encode_rgba16_files_batch at (16, 2)", lambda: png16.png_encode_rgba16_files_batch(wide, off16, files, f_off, width, 2))))
log.close()
