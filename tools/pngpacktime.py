"""Times the encode side from RGBA8 -- fdh_png_pack_batch, fdh_png_analyse_batch and png_encode_rgba_files_batch -- on
n images of 341 x 64, each next to the formulation a user would write in torch today and next to
fdh_png_expand_batch on the same pixels in the same run (pack moves the same bytes the other way).

    python tools/pngpacktime.py [--n 65536] [--rounds 5] [--profile]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE; a round times as many calls
as fill half a second.  Per variant: median, minimum and maximum over the rounds (the spread is what a difference must
exceed) and the rate in bytes the algorithm needs (RGBA read + packed pixels written).
--profile runs every kernel three times and nothing else: for `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import functools
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import synth  # noqa: E402
import timing  # noqa: E402
from timing import interleaved  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
dev = "cuda"
show = functools.partial(timing.show, fmt="%-58s median %9.3f ms, min %9.3f, max %9.3f over %d rounds of %d calls, %.0f GB/s")


def measure(title, variants, nbytes, checks):
    if args.profile:
        for name, f in variants:
            if not name.startswith("torch"):
                for _ in range(3):
                    f()
        torch.cuda.synchronize()
        print("%s: three calls of every kernel" % title)
        return
    ts, calls = interleaved(variants, args.rounds)
    print("%s; %s" % (title, checks))
    med = {name: show("  " + name, ts[name], calls[name], nbytes) for name, _ in variants}
    names = [name for name, _ in variants]
    for other in names[1:]:
        print("  %s / %s = %.2f" % (other, names[0], med[other] / med[names[0]]))
    sys.stdout.flush()


n, L = args.n, 65536
rb, bpp, width = synth.ROW_BYTES - 1, 3, (synth.ROW_BYTES - 1) // 3
rows = L // synth.ROW_BYTES
assert (width, rows) == (341, 64)
raw = synth.gen_batch_torch(0, n, L, model="D", device=dev)
r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
rgb = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
fd.png_unfilter_batch(raw.view(-1), r_off, rgb, p_off, rb, bpp)       # the bench's pixels: runs, gradients and noise
del raw
a_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * width * 4)
rgba = torch.empty(n * rows * width * 4, dtype=torch.uint8, device=dev)
st = torch.empty(n, dtype=torch.int32, device=dev)
fd.png_expand_batch(rgb, p_off, rgba, a_off, width, 8, 2)
torch.cuda.synchronize()

# ---- RGBA8 -> RGB8 ----
packed = torch.empty_like(rgb)


def torch_rgb():
    return rgba.view(n, rows, width, 4)[..., :3].contiguous()


variants = (("fdh_png_pack_batch (RGB8)", lambda: fd.png_pack_batch(rgba, a_off, packed, p_off, width, 8, 2, png_status=st)),
            ("torch: [..., :3].contiguous()", torch_rgb),
            ("fdh_png_expand_batch (RGB8)", lambda: fd.png_expand_batch(rgb, p_off, rgba, a_off, width, 8, 2, png_status=st)))
variants[0][1]()
torch.cuda.synchronize()
same = torch.equal(packed, rgb) and int(st.abs().sum()) == 0
measure("%d x (341 x 64) RGBA8 -> RGB8 -- %.2f GB read, %.2f GB written" % (n, rgba.numel() / 1e9, rgb.numel() / 1e9), variants,
        rgba.numel() + rgb.numel(), "same bytes as the source and status 0: %s" % same)

# ---- RGBA8 of at most 256 colours -> sorted palette + palette-8 ----
g = torch.Generator(device=dev)
g.manual_seed(1)
PAL = torch.unique(torch.randint(-(1 << 31), 1 << 31, (400,), dtype=torch.int64, device=dev, generator=g))[:256]
PAL = PAL[torch.randperm(256, device=dev, generator=g)].to(torch.int32)
index = rgb.view(n, rows, width, 3)[..., 0].contiguous()             # one byte per pixel, with the picture's runs
i_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * width)
del packed
rgba.view(torch.int32).copy_(PAL[index.view(-1).long()])
torch.cuda.synchronize()
pal = torch.empty((n, 256), dtype=torch.int32, device=dev)
colour = torch.empty((n, 4), dtype=torch.int32, device=dev)
trns_len = torch.empty(n, dtype=torch.int32, device=dev)
summary = torch.empty(n, dtype=torch.int32, device=dev)
ast = torch.empty(n, dtype=torch.int32, device=dev)
idx_out = torch.empty(n * rows * width, dtype=torch.uint8, device=dev)


def analyse():
    return fd.png_analyse_batch(rgba, a_off, width, 256, pal=pal, colour=colour, trns_len=trns_len, summary=summary, png_status=ast)


def pack_pal():
    return fd.png_pack_batch(rgba, a_off, idx_out, i_off, width, 8, 3, pal=pal, colour=colour, upstream=ast, png_status=st)


def analyse_and_pack():
    analyse()
    pack_pal()


SIGN = -(1 << 31)


def torch_palette(chunk=2048):
    """Per image: the sorted distinct words (unsigned order: the sign bit flipped), then every pixel's rank among them,
    2048 images at a time (the sorted copy of the whole batch would not fit next to the rest).  Every chunk is computed;
    the indices of the LAST chunk are returned."""
    out = None
    for a in range(0, n, chunk):
        w = rgba.view(torch.int32).view(n, rows * width)[a:a + chunk] ^ SIGN
        s, _ = w.sort(dim=1)
        first = torch.ones_like(s, dtype=torch.bool)
        first[:, 1:] = s[:, 1:] != s[:, :-1]
        rank = first.cumsum(dim=1) - 1
        table = torch.full((w.shape[0], 257), (1 << 31) - 1, dtype=torch.int32, device=dev)
        table.scatter_(1, torch.where(first, rank, torch.full_like(rank, 256)).clamp(max=256), s)
        out = torch.searchsorted(table[:, :256].contiguous(), w.contiguous()).to(torch.uint8)
    return out


analyse_and_pack()
torch.cuda.synchronize()
back = torch.empty_like(rgba)
fd.png_expand_batch(idx_out, i_off, back, a_off, width, 8, 3, pal=pal, colour=colour)
same = torch.equal(back, rgba) and int(st.abs().sum()) == 0 and torch.equal(torch_palette()[-1], idx_out.view(n, rows * width)[-1])
del back
nbytes = rgba.numel() + idx_out.numel()
variants = (("fdh_png_analyse_batch + fdh_png_pack_batch (palette-8)", analyse_and_pack),
            ("fdh_png_analyse_batch alone", analyse),
            ("fdh_png_pack_batch alone (palette-8)", pack_pal),
            ("torch: sort, unique, searchsorted", torch_palette),
            ("fdh_png_expand_batch (palette-8)", lambda: fd.png_expand_batch(idx_out, i_off, rgba, a_off, width, 8, 3, pal=pal, colour=colour, png_status=st)))
measure("%d x (341 x 64) RGBA8 of up to 256 colours -> palette + indices -- %.2f GB read, %.2f GB written" % (n, rgba.numel() / 1e9, idx_out.numel() / 1e9),
        variants, nbytes, "expand gives the source back, status 0, torch agrees on the last image: %s" % same)
del idx_out, index, pal, colour

# ---- RGBA8 -> RGB8 files ----
fd.png_expand_batch(rgb, p_off, rgba, a_off, width, 8, 2)
slot = (fd.png_file_bound(rows, rb) + 15) & ~15
files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
f_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot
file_len, fst = fd.png_encode_rgba_files_batch(rgba, a_off, files, f_off, width, 8, 2)
torch.cuda.synchronize()
ok = int(fst.abs().sum()) == 0
back, _, _, status, png_status = fd.png_decode_files_rgba_batch(files, f_off, width, 8, 2, file_len=file_len)
torch.cuda.synchronize()
same = ok and torch.equal(back, rgba) and int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0
del back
variants = (("png_encode_rgba_files_batch (RGBA8 -> RGB8 files)", lambda: fd.png_encode_rgba_files_batch(rgba, a_off, files, f_off, width, 8, 2)),
            ("torch [..., :3] + png_encode_files_batch", lambda: fd.png_encode_files_batch(torch_rgb().view(-1), p_off, files, f_off, width, 8, 2)),
            ("png_encode_files_batch on packed RGB8 alone", lambda: fd.png_encode_files_batch(rgb, p_off, files, f_off, width, 8, 2)))
measure("%d x (341 x 64) RGBA8 -> PNG files (%.2f GB of files)" % (n, int(file_len.to(torch.int64).sum()) / 1e9), variants, rgba.numel(),
        "the files decode to the source: %s" % same)
