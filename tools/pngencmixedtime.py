"""Times the calls of "PNG encode: mixed batches" against the per-geometry calls they derive from, at the bench shape
(n x (341 x 64 RGB8) as RGBA8 pictures), and the file pipelines on a genuinely mixed collection.

    python tools/pngencmixedtime.py [--n 65536] [--rounds 5] [--skip-files]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE; a round times as many calls
as fill half a second.  Per variant: median [minimum .. maximum] over the rounds.  The margin a mixed call gets is the
spread (max - min) of the per-geometry call's own rounds in this run.
  (a) analyse, pack, choose, fused filter + encode, frame: mixed / per-geometry on the same uniform images
  (b) a mixed collection of the same pixel count -- eight widths from 100 to 600 times four pairs (RGB8, RGBA8, grey-8,
      grey-alpha-8), the geometries interleaved in blocks of sixteen pictures -- through png_encode_mixed_rgba_files_batch
      in ONE call (the pairs forced, and chosen by the plan) against png_encode_rgba_files_batch run once per geometry on
      that geometry's pictures (what a caller had to do before, the grouping not counted)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import synth  # noqa: E402
import timing  # noqa: E402
from timing import arange_off  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip-files", action="store_true")
args = ap.parse_args()
dev = "cuda"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def compare(title, variants):
    """Prints every variant; the first is the mixed call, the second what it is held against."""
    stats = timing.measure(variants, args.rounds, width=64)
    (m, _, _), (p, plo, phi) = stats[0], stats[1]
    print("  %s: mixed / per-geometry = %.3f (%+.3f ms); margin (the per-geometry call's spread) %.3f ms: %s" %
          (title, m / p, m - p, phi - plo, "inside" if m - p <= phi - plo else "OUTSIDE"))
    sys.stdout.flush()
    return stats


def records(n, width, height, depth, colour):
    info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    info[:, 1], info[:, 2], info[:, 3] = width, height, depth | colour << 8
    return info


def pictures(pix, count, w, h, d, c):
    """count images of packed 8-bit scanlines -> RGBA8 through the library's own expansion."""
    rgba = torch.empty(count * h * w * 4, dtype=torch.uint8, device=dev)
    st = fd.png_expand_batch(pix, arange_off(count, h * fd.png_geometry(w, d, c)[0]), rgba, arange_off(count, h * w * 4), w, d, c)
    assert int(st.abs().sum()) == 0
    return rgba


# ---- (a): the bench's synthetic PNG rows as RGBA8 pictures ----
n, L = args.n, 65536
width, rows, depth, colour = (synth.ROW_BYTES - 1) // 3, L // synth.ROW_BYTES, 8, 2
rb, bpp = fd.png_geometry(width, depth, colour)
filtered = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
pix_off, rgba_off, types_off = arange_off(n, rows * rb), arange_off(n, rows * width * 4), arange_off(n, rows)
pixels = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
fd.png_unfilter_batch(filtered, arange_off(n, L), pixels, pix_off, rb, bpp)
del filtered
rgba = pictures(pixels, n, width, rows, depth, colour)
info = records(n, width, rows, depth, colour)
st = torch.empty(n, dtype=torch.int32, device=dev)
print("%d x (%d x %d RGB8): %d bytes of RGBA8, %d of packed pixels each" % (n, width, rows, rows * width * 4, rows * rb))

out = [torch.empty((n, 256), dtype=torch.int32, device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev),
       torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
out2 = [torch.empty_like(t) for t in out]
st2 = torch.empty_like(st)
analyse_mixed = lambda: fd.png_analyse_mixed_batch(rgba, rgba_off, info, pal=out[0], colour=out[1], trns_len=out[2], summary=out[3], png_status=st)
analyse_one = lambda: fd.png_analyse_batch(rgba, rgba_off, width, pal=out2[0], colour=out2[1], trns_len=out2[2], summary=out2[3], png_status=st2)
analyse_mixed(), analyse_one()
torch.cuda.synchronize()
ok = st2 == 0
print("(a) analysis; the two calls agree: %s" % (torch.equal(st, st2) and torch.equal(out[3], out2[3]) and torch.equal(out[1][ok], out2[1][ok])))
compare("(a) analyse", (("png_analyse_mixed_batch", analyse_mixed), ("png_analyse_batch (per geometry)", analyse_one)))
del out, out2

pix2 = torch.empty_like(pixels)
pack_mixed = lambda: fd.png_pack_mixed_batch(rgba, rgba_off, pix2, pix_off, info, png_status=st)
pack_one = lambda: fd.png_pack_batch(rgba, rgba_off, pix2, pix_off, width, depth, colour, png_status=st)
pack_mixed()
torch.cuda.synchronize()
print("(a) packing; the source back: %s" % (int(st.abs().sum()) == 0 and torch.equal(pix2, pixels)))
compare("(a) pack", (("png_pack_mixed_batch", pack_mixed), ("png_pack_batch (per geometry)", pack_one)))
del pix2, rgba

types, types2 = torch.empty(n * rows, dtype=torch.uint8, device=dev), torch.empty(n * rows, dtype=torch.uint8, device=dev)
choose_mixed = lambda: fd.png_choose_filters_mixed_batch(pixels, pix_off, types, types_off, info, png_status=st)
choose_one = lambda: fd.png_choose_filters_batch(pixels, pix_off, types2, types_off, rb, bpp, png_status=st)
choose_mixed(), choose_one()
torch.cuda.synchronize()
print("(a) filter selection; the two calls agree: %s" % torch.equal(types, types2))
compare("(a) choose", (("png_choose_filters_mixed_batch", choose_mixed), ("png_choose_filters_batch (per geometry)", choose_one)))

slot = (fd.png_file_bound(rows, rb) + 15) & ~15
f_off = arange_off(n, slot)
e_off = f_off + fd.PNG_FILE_PREFIX
e_off[n] = f_off[n] - fd.PNG_FILE_SUFFIX
files, files2 = torch.zeros(n * slot, dtype=torch.uint8, device=dev), torch.zeros(n * slot, dtype=torch.uint8, device=dev)
o_len = torch.empty(n, dtype=torch.int32, device=dev)
enc_mixed = lambda: fd.png_filter_deflate_ultrafast_mixed_batch(pixels, pix_off, types, types_off, files, e_off, info, out_len=o_len, png_status=st)
enc_one = lambda: fd.png_filter_deflate_ultrafast_batch(pixels, pix_off, types, types_off, files2, e_off, rb, bpp)
enc_mixed()
o_len2, _ = enc_one()
torch.cuda.synchronize()
print("(a) filter + encode; the two calls agree: %s" % (torch.equal(o_len, o_len2) and torch.equal(files, files2)))
compare("(a) encode", (("png_filter_deflate_ultrafast_mixed_batch", enc_mixed), ("png_filter_deflate_ultrafast_batch (per geometry)", enc_one)))

heights = torch.full((n,), rows, dtype=torch.int32, device=dev)
f_len, f_len2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
frame_mixed = lambda: fd.png_frame_mixed_batch(files, f_off, o_len, info, file_len=f_len, png_status=st)
frame_one = lambda: fd.png_frame_batch(files2, f_off, o_len, heights, width, depth, colour, file_len=f_len2, png_status=st)
frame_mixed(), frame_one()
torch.cuda.synchronize()
print("(a) framing; the two calls agree: %s" % (torch.equal(f_len, f_len2) and torch.equal(files, files2)))
compare("(a) frame", (("png_frame_mixed_batch", frame_mixed), ("png_frame_batch (per geometry)", frame_one)))
del files, files2, types, types2, pixels
if args.skip_files:
    sys.exit(0)

# ---- (b): a mixed collection ----
widths = (100, 171, 243, 314, 386, 457, 529, 600)
pairs = ((8, 2), (8, 6), (8, 0), (8, 4))
BLOCK = 16
per = max(BLOCK, int(n * width / (sum(widths) / len(widths)) / (len(widths) * len(pairs))) // BLOCK * BLOCK)
g = torch.Generator(device=dev)
g.manual_seed(5)
groups = []
for w, (d, c) in ((w, p) for w in widths for p in pairs):
    row_bytes = fd.png_geometry(w, d, c)[0]
    # pictures that compress like the bench's: smooth rows plus a little noise
    base = (torch.arange(rows * row_bytes, device=dev) // 7 % 251).to(torch.uint8)
    pix = (base[None, :] + torch.randint(0, 3, (per, rows * row_bytes), generator=g, device=dev, dtype=torch.uint8)).view(-1)
    groups.append((w, d, c, pictures(pix, per, w, rows, d, c)))
G = len(groups)
order = [(b, k) for b in range(per // BLOCK) for k in range(G)]
mixed = torch.cat([groups[k][3][b * BLOCK * rows * groups[k][0] * 4:(b + 1) * BLOCK * rows * groups[k][0] * 4] for b, k in order])
m_width = torch.tensor([groups[k][0] for b, k in order], dtype=torch.int32, device=dev).repeat_interleave(BLOCK)
m_pairs = torch.tensor([[groups[k][1], groups[k][2]] for b, k in order], dtype=torch.int32, device=dev).repeat_interleave(BLOCK, dim=0)
N = m_width.numel()
m_height = torch.full((N,), rows, dtype=torch.int32, device=dev)
m_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
torch.cumsum(m_width.to(torch.int64) * rows * 4, 0, out=m_off[1:])
r = fd.png_encode_mixed_rgba_files_batch(mixed, m_off, m_width, m_height, pairs=m_pairs)
back = fd.png_decode_mixed_files_rgba_batch(r[0], r[1], file_len=r[2])
torch.cuda.synchronize()
print("(b) %d pictures of %d geometries (%.2f GB of RGBA8, %.0f Mpixel, the bench shape has %.0f): %d encoded, decoded back to the input: %s"
      % (N, G, mixed.numel() / 1e9, mixed.numel() / 4e6, n * width * rows / 1e6, int((r[3] == 0).sum()), torch.equal(back[0], mixed)))
chosen = fd.png_encode_mixed_rgba_files_batch(mixed, m_off, m_width, m_height)
torch.cuda.synchronize()
print("    file bytes: %.3f GB with the pairs forced, %.3f GB with the pairs chosen by the plan" %
      (int(r[2].to(torch.int64).sum()) / 1e9, int(chosen[2].to(torch.int64).sum()) / 1e9))
del r, back, chosen
slots = []
for w, d, c, _ in groups:
    s = (fd.png_file_bound(rows, fd.png_geometry(w, d, c)[0]) + 15) & ~15
    slots.append((torch.zeros(per * s, dtype=torch.uint8, device=dev), arange_off(per, s), arange_off(per, rows * w * 4)))


def per_geometry():
    for (w, d, c, px), (file, off, p_off) in zip(groups, slots):
        fd.png_encode_rgba_files_batch(px, p_off, file, off, w, d, c)


compare("(b)", (("png_encode_mixed_rgba_files_batch, one call, pairs forced", lambda: fd.png_encode_mixed_rgba_files_batch(mixed, m_off, m_width, m_height, pairs=m_pairs)),
                ("png_encode_rgba_files_batch, once per geometry (%d calls)" % G, per_geometry),
                ("png_encode_mixed_rgba_files_batch, one call, pairs chosen", lambda: fd.png_encode_mixed_rgba_files_batch(mixed, m_off, m_width, m_height))))
