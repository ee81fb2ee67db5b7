"""Times the calls of "PNG decode: mixed batches" against the per-geometry calls they derive from, at the bench shape
(n x (341 x 64 RGB8)), and the two file pipelines on a uniform and on a genuinely mixed collection.

    python tools/pngmixedtime.py [--n 65536] [--rounds 5] [--skip-files]

Device events, two warm-up calls each, then `rounds` rounds in which the variants ALTERNATE; a round times as many calls
as fill half a second.  Per variant: median [minimum .. maximum] over the rounds -- the spread is what a difference must
exceed.
  (a) png_expand_mixed_batch / png_expand_batch
  (b) png_unfilter_mixed_batch / png_unfilter_interlaced_batch, method 0 and method 1; png_unfilter_batch for orientation
  (c) gather and colour, mixed / per-geometry
  (d) files -> RGBA8: route="mixed", route="uniform", png_decode_files_rgba_batch
  (e) a mixed collection of the same pixel count -- eight widths from 100 to 600, four pairs, a quarter interlaced, the
      geometries interleaved in blocks of sixteen files -- in ONE mixed call against png_decode_files_rgba_batch run once
      per distinct geometry over the whole batch (what a caller had to do before)
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
from timing import arange_off  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip-files", action="store_true")
args = ap.parse_args()
dev = "cuda"
compare = functools.partial(timing.compare, rounds=args.rounds)
X0, Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
DX, DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def records(n, width, height, depth, colour, interlace, idat_bytes=0):
    info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    info[:, 1], info[:, 2], info[:, 3], info[:, 4], info[:, 5], info[:, 6], info[:, 7] = width, height, depth | colour << 8 | interlace << 16, idat_bytes, 1, 33, 3
    return info


def interlaced_streams(pixels, n, width, rows, ch):
    """The decoded IDAT streams of the pictures stored with Adam7, every pass row with filter type 0."""
    picture = pixels.view(n, rows, width, ch)
    parts = []
    for p in range(7):
        sub = picture[:, Y0[p]::DY[p], X0[p]::DX[p], :]
        if sub.shape[1] and sub.shape[2]:
            body = sub.reshape(n, sub.shape[1], sub.shape[2] * ch)
            parts.append(torch.cat((torch.zeros((n, sub.shape[1], 1), dtype=torch.uint8, device=dev), body), dim=2).view(n, -1))
    return torch.cat(parts, dim=1).contiguous()


# ---- (a), (b): the bench's synthetic PNG rows ----
n, L = args.n, 65536
width, rows, depth, colour = (synth.ROW_BYTES - 1) // 3, L // synth.ROW_BYTES, 8, 2
rb, bpp = fd.png_geometry(width, depth, colour)
progressive = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
prog_off, pix_off, rgba_off = arange_off(n, L), arange_off(n, rows * rb), arange_off(n, rows * width * 4)
pixels = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
fd.png_unfilter_batch(progressive, prog_off, pixels, pix_off, rb, bpp)
size = fd.png_adam7_size(width, rows, depth, colour)
interlaced = interlaced_streams(pixels, n, width, rows, 3).view(-1)
assert interlaced.numel() == n * size
int_off = arange_off(n, size)
info0, info1 = records(n, width, rows, depth, colour, 0), records(n, width, rows, depth, colour, 1)
st = torch.empty(n, dtype=torch.int32, device=dev)
zeros, ones = torch.zeros(n, dtype=torch.uint8, device=dev), torch.ones(n, dtype=torch.uint8, device=dev)
out = torch.empty_like(pixels)
rgba = torch.empty(n * rows * width * 4, dtype=torch.uint8, device=dev)
rgba2 = torch.empty_like(rgba)
print("%d x (%d x %d RGB8): %d bytes progressive, %d interlaced, %d of pixels, %d of RGBA8 each" % (n, width, rows, L, size, rows * rb, rows * width * 4))

fd.png_expand_mixed_batch(pixels, pix_off, rgba, rgba_off, info0, png_status=st)
fd.png_expand_batch(pixels, pix_off, rgba2, rgba_off, width, depth, colour)
torch.cuda.synchronize()
print("(a) expansion; the two calls agree: %s" % (int(st.abs().sum()) == 0 and torch.equal(rgba, rgba2)))
compare("(a)", (("png_expand_mixed_batch", lambda: fd.png_expand_mixed_batch(pixels, pix_off, rgba, rgba_off, info0, png_status=st)),
                ("png_expand_batch (per geometry)", lambda: fd.png_expand_batch(pixels, pix_off, rgba2, rgba_off, width, depth, colour, png_status=st))))
del rgba, rgba2

work0, work1 = progressive.clone(), interlaced.clone()
fd.png_unfilter_mixed_batch(work0, prog_off, out, pix_off, info0, png_status=st)
torch.cuda.synchronize()
same0 = int(st.abs().sum()) == 0 and torch.equal(out, pixels)
out.zero_()
fd.png_unfilter_mixed_batch(work1, int_off, out, pix_off, info1, png_status=st)
torch.cuda.synchronize()
print("(b) reconstruction; the source back: method 0 %s, method 1 %s (from the second call on a call runs over bytes it has already "
      "reconstructed: the work does not depend on the values)" % (same0, int(st.abs().sum()) == 0 and torch.equal(out, pixels)))
compare("(b) method 0", (("png_unfilter_mixed_batch, progressive", lambda: fd.png_unfilter_mixed_batch(work0, prog_off, out, pix_off, info0, png_status=st)),
                         ("png_unfilter_interlaced_batch, method 0", lambda: fd.png_unfilter_interlaced_batch(work0, prog_off, out, pix_off, width, depth, colour, method=zeros, png_status=st)),
                         ("png_unfilter_batch (orientation)", lambda: fd.png_unfilter_batch(progressive, prog_off, out, pix_off, rb, bpp, png_status=st))))
compare("(b) method 1", (("png_unfilter_mixed_batch, Adam7", lambda: fd.png_unfilter_mixed_batch(work1, int_off, out, pix_off, info1, png_status=st)),
                         ("png_unfilter_interlaced_batch, method 1", lambda: fd.png_unfilter_interlaced_batch(work1, int_off, out, pix_off, width, depth, colour, method=ones, png_status=st))))
del work0, work1, out, progressive, interlaced
if args.skip_files:
    sys.exit(0)


# ---- files ----
def encode(pix, count, w, h, d, c, interlace):
    """count pictures -> (file buffer, slot size, file_len): progressive through png_encode_files_batch, interlaced through
    the ultra-fast encoder over the interlaced stream and png_frame_batch with the IHDR's interlace byte and CRC patched."""
    row_bytes = fd.png_geometry(w, d, c)[0]
    slot = (fd.png_file_bound(2 * h, row_bytes) + 15) & ~15
    off = arange_off(count, slot)
    files = torch.zeros(count * slot + 64, dtype=torch.uint8, device=dev)
    p_off = arange_off(count, h * row_bytes)
    if not interlace:
        length, status, _ = fd.png_encode_files_batch(pix, p_off, files, off, w, d, c)
    else:
        stream = interlaced_streams(pix, count, w, h, CHANNELS[c] * d // 8)
        enc_off = off + fd.PNG_FILE_PREFIX
        enc_off[count] = off[count] - fd.PNG_FILE_SUFFIX
        idat_len = fd.deflate_ultrafast_batch(stream.view(-1), arange_off(count, stream.shape[1]), files, enc_off)
        length, status = fd.png_frame_batch(files, off, idat_len, torch.full((count,), h, dtype=torch.int32, device=dev), w, d, c)
        ihdr = b"IHDR" + w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([d, c, 0, 0, 1])
        files[:count * slot].view(count, slot)[:, 28:33] = torch.tensor(list(ihdr[-1:] + zlib.crc32(ihdr).to_bytes(4, "big")), dtype=torch.uint8, device=dev)
    assert int(status.abs().sum()) == 0
    return files[:count * slot], slot, length


files, slot, f_len = encode(pixels, n, width, rows, depth, colour, 0)
f_off = arange_off(n, slot)
info = fd.png_scan_files_batch(files, f_off, f_len)
comp = torch.empty(int(f_len.to(torch.int64).sum()), dtype=torch.uint8, device=dev)
comp_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
torch.cumsum(info[:, 4].to(torch.int64), 0, out=comp_off[1:])
pal = torch.empty((n, 256), dtype=torch.int32, device=dev)
col = torch.empty((n, 4), dtype=torch.int32, device=dev)
clen = torch.empty(n, dtype=torch.int32, device=dev)
print("(c) gather and colour on %d files of %.2f GB" % (n, int(f_len.to(torch.int64).sum()) / 1e9))
compare("(c) gather", (("png_gather_idat_mixed_batch", lambda: fd.png_gather_idat_mixed_batch(files, f_off, info, comp, comp_off, comp_len=clen, png_status=st)),
                       ("png_gather_idat_batch", lambda: fd.png_gather_idat_batch(files, f_off, info, comp, comp_off, width, depth, colour, comp_len=clen, png_status=st))))
compare("(c) colour", (("png_colour_mixed_batch", lambda: fd.png_colour_mixed_batch(files, f_off, info, pal=pal, colour=col, png_status=st)),
                       ("png_colour_batch", lambda: fd.png_colour_batch(files, f_off, info, width, depth, colour, colour=col, png_status=st))))
del comp, pal

a = fd.png_decode_mixed_files_rgba_batch(files, f_off, f_len, route="mixed")
b = fd.png_decode_files_rgba_batch(files, f_off, width, depth, colour, file_len=f_len)
torch.cuda.synchronize()
print("(d) files -> RGBA8; route=\"mixed\" and the per-geometry pipeline agree: %s" % all(torch.equal(x, y) for x, y in zip(a, b)))
del a, b
stats = compare("(d) mixed route", (("png_decode_mixed_files_rgba_batch, route=\"mixed\"", lambda: fd.png_decode_mixed_files_rgba_batch(files, f_off, f_len, route="mixed")),
                            ("png_decode_files_rgba_batch", lambda: fd.png_decode_files_rgba_batch(files, f_off, width, depth, colour, file_len=f_len)),
                            ("png_decode_mixed_files_rgba_batch, route=\"uniform\"", lambda: fd.png_decode_mixed_files_rgba_batch(files, f_off, f_len, route="uniform")),
                            ("png_decode_mixed_files_rgba_batch (route chosen)", lambda: fd.png_decode_mixed_files_rgba_batch(files, f_off, f_len))))
(u, ulo, uhi), (p, plo, phi) = stats[2], stats[1]
print("  (d) route=\"uniform\" %.3f ms against the per-geometry pipeline's [%.3f .. %.3f]: %s" % (u, plo, phi, "inside" if plo <= u <= phi else "outside"))
del files, pixels

# ---- (e): a mixed collection ----
widths = (100, 171, 243, 314, 386, 457, 529, 600)
pairs = ((8, 2), (8, 6), (8, 0), (8, 4))
BLOCK = 16
per = max(BLOCK, int(n * width / (sum(widths) / len(widths)) / (len(widths) * len(pairs))) // BLOCK * BLOCK)
parts, geometries = [], []
g = torch.Generator(device=dev)
g.manual_seed(5)
for k, (w, (d, c)) in enumerate((w, p) for w in widths for p in pairs):
    row_bytes = fd.png_geometry(w, d, c)[0]
    # pictures that compress like the bench's: smooth rows plus a little noise
    base = (torch.arange(rows * row_bytes, device=dev) // 7 % 251).to(torch.uint8)
    pix = (base[None, :] + torch.randint(0, 3, (per, rows * row_bytes), generator=g, device=dev, dtype=torch.uint8)).view(-1)
    parts.append(encode(pix, per, w, rows, d, c, 1 if k % 4 == 3 else 0))
    geometries.append((w, d, c))
G = len(parts)
order = [(b, k) for b in range(per // BLOCK) for k in range(G)]
mixed = torch.cat([parts[k][0][b * BLOCK * parts[k][1]:(b + 1) * BLOCK * parts[k][1]] for b, k in order] + [torch.zeros(64, dtype=torch.uint8, device=dev)])
m_len = torch.cat([parts[k][2][b * BLOCK:(b + 1) * BLOCK] for b, k in order])
slots = torch.tensor([parts[k][1] for b, k in order], dtype=torch.int64, device=dev).repeat_interleave(BLOCK)
m_off = torch.zeros(slots.numel() + 1, dtype=torch.int64, device=dev)
torch.cumsum(slots, 0, out=m_off[1:])
del parts
N = m_len.numel()
A = fd.PNG_FLAG_ADAM7
r = fd.png_decode_mixed_files_rgba_batch(mixed, m_off, m_len, flags=A)
torch.cuda.synchronize()
total_px = r[0].numel() // 4
good = int((r[4] == 0).sum())
# the per-geometry pipeline gives the same pictures, geometry by geometry
agree = True
for w, d, c in geometries:
    q = fd.png_decode_files_rgba_batch(mixed, m_off, w, d, c, file_len=m_len, flags=A)
    mine = (q[4] == 0).nonzero().view(-1).tolist()
    qo, ro = q[1].tolist(), r[1].tolist()
    agree = agree and len(mine) == per and all(torch.equal(q[0][qo[i]:qo[i + 1]], r[0][ro[i]:ro[i + 1]]) for i in mine[::97])
print("(e) %d files of %d geometries (%.2f GB, %.0f Mpixel, the bench shape has %.0f), a quarter interlaced: %d decoded, the per-geometry "
      "pipeline agrees on a sample: %s" % (N, G, int(m_len.to(torch.int64).sum()) / 1e9, total_px / 1e6, n * width * rows / 1e6, good, agree))
del r, q


def per_geometry():
    for w, d, c in geometries:
        fd.png_decode_files_rgba_batch(mixed, m_off, w, d, c, file_len=m_len, flags=A)


compare("(e)", (("png_decode_mixed_files_rgba_batch, one call", lambda: fd.png_decode_mixed_files_rgba_batch(mixed, m_off, m_len, flags=A)),
                ("png_decode_files_rgba_batch, once per geometry (%d calls)" % G, per_geometry)))
