"""Times fdh_png_expand_batch against the formulation a user would write in torch today, on four shapes, and the
end-to-end call png_decode_files_rgba_batch next to png_decode_files_batch on the same files.

    python tools/pngexpandtime.py [--n 65536] [--big 16] [--rounds 5] [--profile] [--skip-files]

Device events, two warm-up calls each, then `rounds` rounds in which the kernel and the torch formulation ALTERNATE;
a round times as many calls as fill half a second.  Per variant: median, minimum and maximum over the rounds (the spread
is what a difference must exceed) and the rate in bytes the algorithm needs (packed pixels read + RGBA written).
--profile runs every kernel three times and nothing else: for `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import synth  # noqa: E402
from timing import interleaved, show  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--big", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--skip-files", action="store_true")
args = ap.parse_args()
dev = "cuda"


def shape(title, n, width, rows, depth, colour, torch_formulation, pal=None):
    """One shape: n images of width x rows; torch_formulation(pix [n, rows, row_bytes] uint8) -> [n, rows, width, 4]."""
    rb, _ = fd.png_geometry(width, depth, colour)
    pix = torch.randint(0, 256, (n, rows, rb), dtype=torch.uint8, device=dev)
    p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * width * 4)
    rgba = torch.empty(n * rows * width * 4, dtype=torch.uint8, device=dev)
    pals = colour_words = None
    if pal is not None:
        pals = pal.view(torch.int32).view(1, 256).repeat(n, 1).contiguous()
        colour_words = torch.tensor([256, 0, 0, 0], dtype=torch.int32, device=dev).repeat(n, 1).contiguous()
    st = torch.empty(n, dtype=torch.int32, device=dev)

    def kernel():
        return fd.png_expand_batch(pix.view(-1), p_off, rgba, r_off, width, depth, colour, pal=pals, colour=colour_words, png_status=st)

    nbytes = n * rows * (rb + width * 4)
    if args.profile:
        for _ in range(3):
            kernel()
        torch.cuda.synchronize()
        print("%s: three calls, %d bytes each" % (title, nbytes))
        return
    kernel()
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    few = min(n, 8)
    same = torch.equal(rgba[:few * rows * width * 4].view(few, rows, width, 4), torch_formulation(pix[:few]))
    ts, calls = interleaved((("kernel", kernel), ("torch", lambda: torch_formulation(pix))), args.rounds)
    print("%s -- %.2f GB read, %.2f GB written; same pixels as torch: %s" % (title, n * rows * rb / 1e9, n * rows * width * 4 / 1e9, same))
    k = show("  fdh_png_expand_batch", ts["kernel"], calls["kernel"], nbytes)
    t = show("  torch formulation", ts["torch"], calls["torch"], nbytes)
    print("  torch / kernel = %.2f" % (t / k))


def rgb8(pix):
    n, rows, rb = pix.shape
    x = pix.view(n, rows, rb // 3, 3)
    return torch.cat([x, torch.full((n, rows, rb // 3, 1), 255, dtype=torch.uint8, device=dev)], dim=3)


PAL = torch.randint(0, 256, (256, 4), dtype=torch.uint8, device=dev)


def pal8(pix):
    return PAL[pix.long()]


SHIFTS = torch.arange(7, -1, -1, dtype=torch.uint8, device=dev)


def grey1(pix, chunk=2048):
    """Shifts and masks, 2048 images at a time (the unpacked bits of the whole batch would not fit next to the result)."""
    n, rows, rb = pix.shape
    out = None
    for a in range(0, n, chunk):
        x = pix[a:a + chunk]
        g = (((x.unsqueeze(-1) >> SHIFTS) & 1) * 255).view(x.shape[0], rows, rb * 8)
        out = torch.stack([g, g, g, torch.full_like(g, 255)], dim=-1)
    return out


def rgba16(pix):
    n, rows, rb = pix.shape
    return pix.view(n, rows, rb // 8, 4, 2)[..., 0].contiguous()


for title, shape_args in (("%d x (341 x 64 RGB8)" % args.n, (args.n, 341, 64, 8, 2, rgb8)),
                          ("%d x (1023 x 64 palette-8)" % args.n, (args.n, 1023, 64, 8, 3, pal8, PAL)),
                          ("%d x (8184 x 64 one-bit grey)" % args.n, (args.n, 8184, 64, 1, 0, grey1)),
                          ("%d x (8192 x 8192 RGBA16)" % args.big, (args.big, 8192, 8192, 16, 6, rgba16))):
    try:
        shape(title, *shape_args)
    except torch.OutOfMemoryError as e:
        print("%s: not measured, out of device memory (%s)" % (title, str(e).split(".")[0]))
    sys.stdout.flush()
    torch.cuda.empty_cache()

if not args.skip_files and not args.profile:
    # files in -> RGBA out at the first shape, next to files in -> packed pixels: what the added step costs
    n, L = args.n, 65536
    raw = synth.gen_batch_torch(0, n, L, model="D", device=dev)
    rb, bpp, width = synth.ROW_BYTES - 1, 3, (synth.ROW_BYTES - 1) // 3
    rows = L // synth.ROW_BYTES
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
    pixels = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
    fd.png_unfilter_batch(raw.view(-1), r_off, pixels, p_off, rb, bpp)
    slot = (fd.png_file_bound(rows, rb) + 15) & ~15
    files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    f_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot
    file_len, st, _ = fd.png_encode_files_batch(pixels, p_off, files, f_off, width, 8, 2)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    del raw
    rgba, rgba_off, _, status, png_status = fd.png_decode_files_rgba_batch(files, f_off, width, 8, 2, file_len=file_len)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0
    same = torch.equal(rgba.view(n, rows, width, 4)[..., :3].contiguous().view(-1), pixels) and bool((rgba.view(-1, 4)[:, 3] == 255).all())
    del rgba
    variants = (("files -> packed pixels (png_decode_files_batch)", lambda: fd.png_decode_files_batch(files, f_off, width, 8, 2, file_len=file_len)),
                ("files -> RGBA8 (png_decode_files_rgba_batch)", lambda: fd.png_decode_files_rgba_batch(files, f_off, width, 8, 2, file_len=file_len)))
    ts, calls = interleaved(variants, args.rounds)
    print("%d files of %d x %d RGB8 (%.2f GB of files); RGBA gives the source back: %s" % (n, width, rows, int(file_len.to(torch.int64).sum()) / 1e9, same))
    med = [show("  " + name, ts[name], calls[name], n * rows * rb) for name, _ in variants]
    print("  the added step costs %.3f ms (%.1f %%)" % (med[1] - med[0], 100 * (med[1] - med[0]) / med[0]))
