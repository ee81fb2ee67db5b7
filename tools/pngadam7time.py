"""Times fdh_png_unfilter_interlaced_batch on n x (341 x 64 RGB8) against fdh_png_unfilter_batch on the same pictures
stored progressively (the same reconstruction work without the placement) and against the placement written in torch
(strided slice assignment per pass), and the two file pipelines on interlaced and on progressive files of the same
pictures, with and without PNG_FLAG_ADAM7.

    python tools/pngadam7time.py [--n 65536] [--rounds 5] [--profile] [--skip-files]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE; a round times as many calls
as fill half a second.  Per variant: median, minimum and maximum over the rounds (the spread is what a difference must
exceed) and the rate in bytes the algorithm needs (decoded stream read + packed pixels written).  The new call
reconstructs in place, so from its second call on it runs over bytes it has already reconstructed: the kernels' work does
not depend on the values (every predictor is computed for every byte), and the first call is checked against the source.
--profile runs every kernel three times and nothing else: for `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import functools
import os
import sys
import zlib

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import synth  # noqa: E402
import timing  # noqa: E402
from timing import arange_off, interleaved  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--skip-files", action="store_true")
args = ap.parse_args()
dev = "cuda"
show = functools.partial(timing.show, fmt="%-66s median %8.3f ms, min %8.3f, max %8.3f over %d rounds of %d calls, %.0f GB/s")
X0, Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
DX, DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)


# ---- the pictures: the bench's synthetic PNG rows, reconstructed ----
n, L = args.n, 65536
width, rows, depth, colour = (synth.ROW_BYTES - 1) // 3, L // synth.ROW_BYTES, 8, 2
rb, bpp = fd.png_geometry(width, depth, colour)
progressive = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)     # rows x (1 + rb) filtered bytes per image
prog_off = arange_off(n, L)
pix_off = arange_off(n, rows * rb)
pixels = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
fd.png_unfilter_batch(progressive, prog_off, pixels, pix_off, rb, bpp)

# ---- the same pictures interlaced: every pass filtered as an image of its own, with the types the chooser picks ----
size = fd.png_adam7_size(width, rows, depth, colour)
passes = [(len(range(X0[p], width, DX[p])), len(range(Y0[p], rows, DY[p]))) for p in range(7)]
picture = pixels.view(n, rows, width, 3)
parts = []
for p, (pw, ph) in enumerate(passes):
    sub = picture[:, Y0[p]::DY[p], X0[p]::DX[p], :].contiguous().view(-1)
    types = torch.empty(n * ph, dtype=torch.uint8, device=dev)
    t_off, s_off, f_off = arange_off(n, ph), arange_off(n, ph * pw * 3), arange_off(n, ph * (pw * 3 + 1))
    fd.png_choose_filters_batch(sub, s_off, types, t_off, pw * 3, bpp)
    filt = torch.empty(n * ph * (pw * 3 + 1), dtype=torch.uint8, device=dev)
    st = fd.png_filter_batch(sub, s_off, types, t_off, filt, f_off, pw * 3, bpp)
    assert int(st.abs().sum()) == 0
    parts.append(filt.view(n, -1))
interlaced = torch.cat(parts, dim=1).contiguous().view(-1)
del parts, sub, filt
assert interlaced.numel() == n * size
int_off = arange_off(n, size)
work = interlaced.clone()
out = torch.empty_like(pixels)
st = torch.empty(n, dtype=torch.int32, device=dev)
ones = torch.ones(n, dtype=torch.uint8, device=dev)
zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
prog_work = progressive.clone()


def adam7():
    return fd.png_unfilter_interlaced_batch(work, int_off, out, pix_off, width, depth, colour, method=ones, png_status=st)


def one_pass():
    return fd.png_unfilter_interlaced_batch(prog_work, prog_off, out, pix_off, width, depth, colour, method=zeros, png_status=st)


def parent():
    return fd.png_unfilter_batch(progressive, prog_off, out, pix_off, rb, bpp, png_status=st)


def torch_placement():
    """From the reconstructed passes in `work` to the picture: one strided slice assignment per pass."""
    dst = out.view(n, rows, width, 3)
    at = 0
    w = work.view(n, size)
    for p, (pw, ph) in enumerate(passes):
        dst[:, Y0[p]::DY[p], X0[p]::DX[p], :] = w[:, at:at + ph * (1 + pw * 3)].view(n, ph, 1 + pw * 3)[:, :, 1:].reshape(n, ph, pw, 3)
        at += ph * (1 + pw * 3)


if args.profile:
    for f in (adam7, one_pass, parent):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    print("three calls each: interlaced, one pass (method 0), fdh_png_unfilter_batch; %d images" % n)
    sys.exit(0)

adam7()
torch.cuda.synchronize()
same = int(st.abs().sum()) == 0 and torch.equal(out, pixels)
out.zero_()
torch_placement()
same_torch = torch.equal(out, pixels)
one_pass()
torch.cuda.synchronize()
same_one = int(st.abs().sum()) == 0 and torch.equal(out, pixels)
print("%d x (%d x %d RGB8): %d bytes interlaced, %d progressive, %d of pixels each; the source back: interlaced %s, torch placement %s, "
      "method 0 %s" % (n, width, rows, size, L, rows * rb, same, same_torch, same_one))
nbytes = n * (size + rows * rb)
variants = (("fdh_png_unfilter_interlaced_batch, Adam7", adam7), ("fdh_png_unfilter_batch, progressive (the parent's)", parent),
            ("fdh_png_unfilter_interlaced_batch, method 0, progressive", one_pass), ("torch placement alone (7 strided assignments)", torch_placement))
ts, calls = interleaved(variants, args.rounds)
med = [show("  " + name, ts[name], calls[name], nbytes) for name, _ in variants]
print("  Adam7 / progressive = %.2f; the placement in torch alone / the whole Adam7 call = %.2f" % (med[0] / med[1], med[3] / med[0]))
sys.stdout.flush()
del work, prog_work, out, progressive

if not args.skip_files:
    # ---- files: progressive ones from png_encode_files_batch; interlaced ones from the ultra-fast encoder over the interlaced
    #      stream and png_frame_batch, the IHDR's interlace byte and CRC patched (they are the same in every file) ----
    slot = (fd.png_file_bound(rows, rb) + 8 * 64 + 15) & ~15
    f_off = arange_off(n, slot)
    prog_files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    prog_len, st1, _ = fd.png_encode_files_batch(pixels, pix_off, prog_files, f_off, width, depth, colour)
    int_files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    enc_off = f_off + fd.PNG_FILE_PREFIX
    enc_off[n] = f_off[n] - fd.PNG_FILE_SUFFIX
    idat_len = fd.deflate_ultrafast_batch(interlaced, int_off, int_files, enc_off)
    height = torch.full((n,), rows, dtype=torch.int32, device=dev)
    int_len, st2 = fd.png_frame_batch(int_files, f_off, idat_len, height, width, depth, colour)
    torch.cuda.synchronize()
    assert int(st1.abs().sum()) == 0 and int(st2.abs().sum()) == 0
    ihdr = b"IHDR" + width.to_bytes(4, "big") + rows.to_bytes(4, "big") + bytes([depth, colour, 0, 0, 1])
    patch = torch.tensor(list(ihdr[-1:] + zlib.crc32(ihdr).to_bytes(4, "big")), dtype=torch.uint8, device=dev)
    int_files[:n * slot].view(n, slot)[:, 28:33] = patch
    del interlaced
    A = fd.PNG_FLAG_ADAM7
    pix2, _, info, status, png_status = fd.png_decode_files_batch(int_files, f_off, width, depth, colour, file_len=int_len, flags=A)
    torch.cuda.synchronize()
    ok = int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0 and torch.equal(pix2, pixels) and bool((info.view(torch.uint8).view(n, 32)[:, 14] == 1).all())
    rgba, _, _, status, png_status = fd.png_decode_files_rgba_batch(int_files, f_off, width, depth, colour, file_len=int_len, flags=A)
    torch.cuda.synchronize()
    ok_rgba = int(png_status.abs().sum()) == 0 and torch.equal(rgba.view(n, rows, width, 4)[..., :3].contiguous().view(-1), pixels)
    del pix2, rgba
    print("%d interlaced files (%.2f GB) and %d progressive ones (%.2f GB) of the same pictures; interlaced files give the source back: "
          "packed %s, RGBA %s" % (n, int(int_len.to(torch.int64).sum()) / 1e9, n, int(prog_len.to(torch.int64).sum()) / 1e9, ok, ok_rgba))

    def dec(files, lens, flags, rgba):
        f = fd.png_decode_files_rgba_batch if rgba else fd.png_decode_files_batch
        return lambda: f(files, f_off, width, depth, colour, file_len=lens, flags=flags)

    variants = (("progressive files -> packed pixels, no flag (the parent's path)", dec(prog_files, prog_len, 0, False)),
                ("progressive files -> packed pixels, PNG_FLAG_ADAM7", dec(prog_files, prog_len, A, False)),
                ("interlaced files  -> packed pixels, PNG_FLAG_ADAM7", dec(int_files, int_len, A, False)),
                ("progressive files -> RGBA8, no flag (the parent's path)", dec(prog_files, prog_len, 0, True)),
                ("progressive files -> RGBA8, PNG_FLAG_ADAM7", dec(prog_files, prog_len, A, True)),
                ("interlaced files  -> RGBA8, PNG_FLAG_ADAM7", dec(int_files, int_len, A, True)))
    ts, calls = interleaved(variants, args.rounds)
    med = [show("  " + name, ts[name], calls[name], n * rows * rb) for name, _ in variants]
    print("  packed: flag on progressive files %+.3f ms; interlaced / progressive = %.2f.  RGBA8: flag %+.3f ms; interlaced / progressive = %.2f"
          % (med[1] - med[0], med[2] / med[0], med[4] - med[3], med[5] / med[3]))
