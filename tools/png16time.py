"""Times the RGBA16 calls of fdeflate_amd.png16 against what each is judged by, in the same run: fdh_png_expand_batch
(RGBA8) on the same pixels, the formulation a user would write in torch today, and the RGBA8 file pipelines on the same
files.

    python tools/png16time.py [--n 65536] [--rounds 5] [--skip-files] [--skip-torch]

Device events, two warm-up calls each, then `rounds` rounds in which the variants of a case ALTERNATE; a round times as
many calls as fill half a second.  Per variant: median, minimum and maximum over the rounds (the spread is what a
difference must exceed) and the rate in bytes the algorithm needs (packed pixels read + picture written, or the
reverse).  FDH_LIB=<another build of the library> measures that build: the two shapes of the wide path
(-DFDH_EXPAND16_GROUP=2 / 4) are compared by running this tool once with each.
"""
import argparse
import functools
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd  # noqa: E402
import fdeflate_amd.png16 as p16  # noqa: E402
from fdeflate_amd import synth  # noqa: E402
import timing  # noqa: E402
from timing import interleaved  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip-files", action="store_true")
ap.add_argument("--skip-torch", action="store_true")
args = ap.parse_args()
dev = "cuda"
show = functools.partial(timing.show, fmt="  %-58s median %9.3f ms, min %9.3f, max %9.3f over %d rounds of %d calls, %5.0f GB/s")
WIDTH, ROWS = 341, 64
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def swap16(pix):
    """Big-endian 16-bit samples (uint8 [..., 2 k]) as int16 in the device's order: the byte swap through an int16 view."""
    v = pix.view(torch.int16)
    return ((v >> 8) & 0xFF) | (v << 8)


def torch_rgba16(pix, depth, colour):
    """What a user has today: png_decode_files_batch's packed pixels [n, rows, row_bytes] to [n, rows, width, 4] int16
    (the bit patterns of the uint16 samples): swap, widen, alpha by torch.cat.  (No key in these shapes: a key would be
    one more comparison over the samples.)"""
    n, rows, _ = pix.shape
    ch = CHANNELS[colour]
    if depth == 16:
        s = swap16(pix).view(n, rows, WIDTH, ch)
    else:
        s = (pix.view(n, rows, WIDTH, ch).to(torch.int16) * 257)
    if colour == 6:
        return s.contiguous()
    opaque = torch.full((n, rows, WIDTH, 1), -1, dtype=torch.int16, device=dev)
    if colour == 2:
        return torch.cat([s, opaque], dim=3)
    if colour == 0:
        return torch.cat([s, s, s, opaque], dim=3)
    return torch.cat([s[..., :1], s[..., :1], s[..., :1], s[..., 1:]], dim=3)


def expand_case(title, n, depth, colour):
    rb, _ = fd.png_geometry(WIDTH, depth, colour)
    pix = torch.randint(0, 256, (n, ROWS, rb), dtype=torch.uint8, device=dev)
    p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * rb)
    r8_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * WIDTH * 4)
    r16_off = r8_off * 2
    rgba8 = torch.empty(n * ROWS * WIDTH * 4, dtype=torch.uint8, device=dev)
    rgba16 = torch.empty(n * ROWS * WIDTH * 8, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)

    def wide():
        return p16.png_expand16_batch(pix.view(-1), p_off, rgba16, r16_off, WIDTH, depth, colour, png_status=st)

    def narrow():
        return fd.png_expand_batch(pix.view(-1), p_off, rgba8, r8_off, WIDTH, depth, colour, png_status=st)

    wide()
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    few = min(n, 8)
    same = torch.equal(rgba16[:few * ROWS * WIDTH * 8].view(torch.int16).view(few, ROWS, WIDTH, 4), torch_rgba16(pix[:few], depth, colour))
    variants = [("fdh_png_expand16_batch -> RGBA16", wide), ("fdh_png_expand_batch -> RGBA8", narrow)]
    if not args.skip_torch:
        variants.append(("torch formulation -> RGBA16", lambda: torch_rgba16(pix, depth, colour)))
    ts, calls = interleaved(variants, args.rounds)
    b16, b8 = n * ROWS * (rb + WIDTH * 8), n * ROWS * (rb + WIDTH * 4)
    print("%s -- %.2f GB read, %.2f GB written as RGBA16; same pixels as torch: %s" % (title, n * ROWS * rb / 1e9, n * ROWS * WIDTH * 8 / 1e9, same))
    w = show(variants[0][0], ts[variants[0][0]], calls[variants[0][0]], b16)
    m = show(variants[1][0], ts[variants[1][0]], calls[variants[1][0]], b8)
    print("  rate of RGBA16 / rate of RGBA8 = %.2f" % ((b16 / w) / (b8 / m)))
    if not args.skip_torch:
        t = show(variants[2][0], ts[variants[2][0]], calls[variants[2][0]], b16)
        print("  torch / kernel = %.2f" % (t / w))
    sys.stdout.flush()


def pack_case(n):
    rb, _ = fd.png_geometry(WIDTH, 16, 2)
    rgba16 = torch.randint(0, 256, (n, ROWS, WIDTH, 8), dtype=torch.uint8, device=dev)
    rgba16[..., 6:] = 255                                                             # A = 65535: RGB16 can hold it
    rgba8 = rgba16[..., 0::2].contiguous()
    rgba8[..., 3] = 255
    r16_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * WIDTH * 8)
    r8_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * WIDTH * 4)
    p16_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * rb)
    p8_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * WIDTH * 3)
    pix16 = torch.empty(n * ROWS * rb, dtype=torch.uint8, device=dev)
    pix8 = torch.empty(n * ROWS * WIDTH * 3, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)

    def wide():
        return p16.png_pack16_batch(rgba16.view(-1), r16_off, pix16, p16_off, WIDTH, 2, png_status=st)

    def narrow():
        return fd.png_pack_batch(rgba8.view(-1), r8_off, pix8, p8_off, WIDTH, 8, 2, png_status=st)

    def formulation():
        return swap16(rgba16.view(n, ROWS, WIDTH, 8)[..., :6].contiguous())

    wide()
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    few = min(n, 8)
    same = torch.equal(pix16[:few * ROWS * rb].view(torch.int16), swap16(rgba16[:few].view(few, ROWS, WIDTH, 8)[..., :6].contiguous()).view(-1))
    variants = [("fdh_png_pack16_batch RGBA16 -> RGB16", wide), ("fdh_png_pack_batch RGBA8 -> RGB8", narrow)]
    if not args.skip_torch:
        variants.append(("torch formulation RGBA16 -> RGB16", formulation))
    ts, calls = interleaved(variants, args.rounds)
    b16, b8 = n * ROWS * WIDTH * (8 + 6), n * ROWS * WIDTH * (4 + 3)
    print("%d x (341 x 64) RGBA16 -> RGB16 -- same bytes as torch: %s" % (n, same))
    w = show(variants[0][0], ts[variants[0][0]], calls[variants[0][0]], b16)
    m = show(variants[1][0], ts[variants[1][0]], calls[variants[1][0]], b8)
    print("  rate of pack16 / rate of pack = %.2f" % ((b16 / w) / (b8 / m)))
    if not args.skip_torch:
        t = show(variants[2][0], ts[variants[2][0]], calls[variants[2][0]], b16)
        print("  torch / kernel = %.2f" % (t / w))
    sys.stdout.flush()


def pictures8(n, seed):
    """n RGB8 pictures of 341 x 64 with the statistics of the bench's model D: its filtered rows, reconstructed."""
    L = 65536
    raw = synth.gen_batch_torch(seed, n, L, model="D", device=dev)
    rb = synth.ROW_BYTES - 1
    rows = L // synth.ROW_BYTES
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
    pixels = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
    fd.png_unfilter_batch(raw.view(-1), r_off, pixels, p_off, rb, 3)
    assert rows == ROWS and rb == WIDTH * 3
    return pixels.view(n, ROWS, WIDTH, 3)


def files_case(n):
    """RGB16 files whose high bytes are one set of model-D pictures and whose low bytes are another: RGBA16 -> files,
    files -> RGBA16 by both pipelines, next to the RGBA8 pipelines and the torch formulation on the same files."""
    hi, lo = pictures8(n, 0), pictures8(n, 1)
    rgba16 = torch.full((n, ROWS, WIDTH, 4, 2), 255, dtype=torch.uint8, device=dev)
    rgba16[..., :3, 0] = lo
    rgba16[..., :3, 1] = hi
    del hi, lo
    rb, _ = fd.png_geometry(WIDTH, 16, 2)
    r16_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (ROWS * WIDTH * 8)
    slot = (fd.png_file_bound(ROWS, rb) + 15) & ~15
    files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
    f_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot

    def encode():
        return p16.png_encode_rgba16_files_batch(rgba16.view(-1), r16_off, files, f_off, WIDTH, 2)

    file_len, st = encode()
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    out = p16.png_decode_files_rgba16_batch(files, f_off, WIDTH, 16, 2, file_len=file_len)
    torch.cuda.synchronize()
    assert int(out[3].abs().sum()) == 0 and int(out[4].abs().sum()) == 0
    same = torch.equal(out[0], rgba16.view(-1))
    del out

    def formulation():
        pix, pix_off, _, _, _ = fd.png_decode_files_batch(files, f_off, WIDTH, 16, 2, file_len=file_len)
        return torch_rgba16(pix.view(n, ROWS, rb), 16, 2)

    variants = [("files -> RGBA16 (png_decode_files_rgba16_batch)", lambda: p16.png_decode_files_rgba16_batch(files, f_off, WIDTH, 16, 2, file_len=file_len)),
                ("files -> RGBA8  (png_decode_files_rgba_batch)", lambda: fd.png_decode_files_rgba_batch(files, f_off, WIDTH, 16, 2, file_len=file_len)),
                ("files -> RGBA16 (png_decode_mixed_files_rgba16_batch, mixed)", lambda: p16.png_decode_mixed_files_rgba16_batch(files, f_off, file_len, route="mixed")),
                ("files -> RGBA8  (png_decode_mixed_files_rgba_batch, mixed)", lambda: fd.png_decode_mixed_files_rgba_batch(files, f_off, file_len, route="mixed")),
                ("files -> packed pixels (png_decode_files_batch)", lambda: fd.png_decode_files_batch(files, f_off, WIDTH, 16, 2, file_len=file_len)),
                ("RGBA16 -> files (png_encode_rgba16_files_batch)", encode)]
    if not args.skip_torch:
        variants.insert(5, ("files -> RGBA16 (png_decode_files_batch + torch formulation)", formulation))
    ts, calls = interleaved(variants, args.rounds)
    print("%d files of %d x %d RGB16 (%.2f GB of files, %.2f GB of pictures); RGBA16 gives the source back: %s"
          % (n, WIDTH, ROWS, int(file_len.to(torch.int64).sum()) / 1e9, n * ROWS * WIDTH * 8 / 1e9, same))
    for name, _ in variants:
        show(name, ts[name], calls[name], n * ROWS * WIDTH * 8)
    sys.stdout.flush()


print("library: %s" % os.environ.get("FDH_LIB", "the package's own"))
for title, depth, colour in (("RGBA16", 16, 6), ("RGB16", 16, 2), ("grey-16", 16, 0), ("RGB8", 8, 2)):
    try:
        expand_case("%d x (341 x 64 %s)" % (args.n, title), args.n, depth, colour)
    except torch.OutOfMemoryError as e:
        print("%s: not measured, out of device memory (%s)" % (title, str(e).split(".")[0]))
    torch.cuda.empty_cache()
pack_case(args.n)
torch.cuda.empty_cache()
if not args.skip_files:
    files_case(args.n)
