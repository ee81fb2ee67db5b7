import os, sys, torch
sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd
from fdeflate_amd import synth
import timing
n, L = 65536, 65536
dev = "cuda"
raw = synth.gen_batch_torch(0, n, L, model="D", device=dev)
r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
rb, bpp = synth.ROW_BYTES - 1, 3
rows = L // synth.ROW_BYTES
p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
pix = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
def step():
    return fd.png_unfilter_batch(raw.view(-1), r_off, pix, p_off, rb, bpp)
st = step(); torch.cuda.synchronize()
assert int(st.abs().sum()) == 0
best = 1e9
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): step()
    e1.record(); torch.cuda.synchronize()
    best = min(best, e0.elapsed_time(e1) / 5)
print("png reconstruction of %d images: %.3f ms (%.0f GB/s of filtered bytes)" % (n, best, n * L / best / 1e6))

# filter -> ultra-fast encode: fused kernel against the two separate calls
types = raw.view(n, rows, rb + 1)[:, :, 0].contiguous().view(-1) % 5
t_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * rows
pixels = pix   # (whatever the reconstruction left there: it is only a byte source)
bound = (fd.ultrafast_bound(L) + 15) & ~15
o_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * bound
enc = torch.empty(n * bound, dtype=torch.uint8, device=dev)
filt = torch.empty(n * L, dtype=torch.uint8, device=dev)


def fused():
    return fd.png_filter_deflate_ultrafast_batch(pixels, p_off, types, t_off, enc, o_off, rb, bpp)


def separate():
    fd.png_filter_batch(pixels, p_off, types, t_off, filt, r_off, rb, bpp)
    return fd.deflate_ultrafast_batch(filt, r_off, enc, o_off)


def best_of(f):
    f(); torch.cuda.synchronize()
    b = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5): f()
        e1.record(); torch.cuda.synchronize()
        b = min(b, e0.elapsed_time(e1) / 5)
    return b


ol_f, st_f = fused(); torch.cuda.synchronize()
enc_f = enc.clone()
ol_s = separate(); torch.cuda.synchronize()
same = bool((ol_f == ol_s).all()) and int(st_f.abs().sum()) == 0
# compare the streams themselves (the slots' tails are not defined)
idx = torch.arange(bound, device=dev).unsqueeze(0) < ol_s.to(torch.int64).unsqueeze(1)
same = same and bool(((enc_f.view(n, bound) == enc.view(n, bound)) | ~idx).all())
tf, ts = best_of(fused), best_of(separate)
print("filter + ultra-fast encode of %d images: fused %.3f ms, separate calls %.3f ms, same streams: %s" % (n, tf, ts, same))

# filter selection (fdh_png_choose_filters_batch) in front of the fused encoder, on the pixels the reconstruction above
# produced: (a) choosing alone, (b) the fused filter + encode alone with the chosen types, (c) both back to back on one
# stream.  Interleaved rounds in this one process, warm; median and minimum per call.
chosen = torch.empty(n * rows, dtype=torch.uint8, device=dev)


def choose():
    return fd.png_choose_filters_batch(pixels, p_off, chosen, t_off, rb, bpp)


def encode_chosen():
    return fd.png_filter_deflate_ultrafast_batch(pixels, p_off, chosen, t_off, enc, o_off, rb, bpp)


def choose_and_encode():
    return fd.png_encode_ultrafast_batch(pixels, p_off, enc, o_off, rb, bpp, types=chosen, types_off=t_off)


assert int(choose().abs().sum()) == 0
variants = (("choose", choose), ("encode", encode_chosen), ("choose + encode", choose_and_encode))
times, _ = timing.interleaved(variants, 9, calls=5)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
for name, _ in variants:
    print("%-16s median %.3f ms, min %.3f ms over %d rounds of 5 calls" % (name, med[name], min(times[name]), len(times[name])))
print("filter selection: %.3f ms = %.0f GB/s of pixels; choose / encode = %.2f" % (med["choose"], n * rows * rb / med["choose"] / 1e6, med["choose"] / med["encode"]))

# what the choice buys: compressed bytes of the batch under the chosen types and under each single type
hist = torch.bincount(chosen.to(torch.int64), minlength=5).tolist()
ol, st = encode_chosen(); torch.cuda.synchronize()
assert int(st.abs().sum()) == 0
total = {"chosen": int(ol.to(torch.int64).sum())}
for t in range(5):
    chosen.fill_(t)
    ol, st = encode_chosen(); torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    total["type %d" % t] = int(ol.to(torch.int64).sum())
print("rows per chosen type (None, Sub, Up, Average, Paeth): %s" % hist)
for k, v in total.items():
    print("compressed bytes, %-7s %14d  (%.4f of the pixels, %.4f of chosen)" % (k + ":", v, v / (n * rows * rb), v / total["chosen"]))

# ---- PNG files: CRC-32 of the encoder's output, the framing, the container scan and the IDAT gather ----
# Interleaved rounds again.  Beside the CRC: a device copy of the encoder's buffer, as this box's memory bandwidth.
import os

width, depth, colour = rb // bpp, 8, 2
assert fd.png_geometry(width, depth, colour) == (rb, bpp)
choose()
ol, st = encode_chosen(); torch.cuda.synchronize()
assert int(st.abs().sum()) == 0
stream_bytes = int(ol.to(torch.int64).sum())


def show(name, t, nbytes=None):
    t = sorted(t)
    rate = "" if nbytes is None else ", %.0f GB/s" % (nbytes / t[len(t) // 2] / 1e6)
    print("%-44s median %.3f ms, min %.3f, max %.3f over %d rounds%s" % (name, t[len(t) // 2], t[0], t[-1], len(t), rate))


big_n = 256 << 20
big = torch.randint(0, 256, (big_n + 16,), dtype=torch.uint8, device=dev)
big_off = torch.tensor([0, big_n], dtype=torch.int64, device=dev)
enc_copy = torch.empty_like(enc)
ts, _ = timing.interleaved((("device copy of the encoder's buffer", lambda: enc_copy.copy_(enc)),), 5, calls=3)
show("device copy, %.2f GB read + as much written" % (enc.numel() / 1e9), ts["device copy of the encoder's buffer"], 2 * enc.numel())
del enc_copy
for copies in ("1", "8", "32"):
    os.environ["FDH_CRC_COPIES"] = copies
    ts, _ = timing.interleaved((("streams", lambda: fd.crc32_batch(enc, o_off, ol)), ("big", lambda: fd.crc32_batch(big, big_off))), 9, calls=5)
    show("crc32 of %d streams (%.2f GB), %s table copies" % (n, stream_bytes / 1e9, copies), ts["streams"], stream_bytes)
    show("crc32 of one 256 MiB range, %s table copies" % copies, ts["big"], big_n)
os.environ.pop("FDH_CRC_COPIES")

slot = (fd.png_file_bound(rows, rb) + 15) & ~15
files = torch.empty(n * slot + 64, dtype=torch.uint8, device=dev)
f_off0 = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot        # the stream starts at +41: not aligned
f_off7 = f_off0 + 7                                                        # the stream starts at +48: 16-byte aligned
enc2 = torch.empty(n * bound + 64, dtype=torch.uint8, device=dev)
o_off41 = o_off + 41
height = torch.full((n,), rows, dtype=torch.int32, device=dev)
file_len, st, _ = fd.png_encode_files_batch(pixels, p_off, files, f_off0, width, depth, colour); torch.cuda.synchronize()
assert int(st.abs().sum()) == 0 and bool((file_len == ol + 57).all())
variants = (
    ("pixels -> streams (choose + encode)", choose_and_encode),
    ("pixels -> files, file_off % 16 == 0", lambda: fd.png_encode_files_batch(pixels, p_off, files, f_off0, width, depth, colour)),
    ("pixels -> files, file_off % 16 == 7", lambda: fd.png_encode_files_batch(pixels, p_off, files, f_off7, width, depth, colour)),
    ("framing alone (prefix, IDAT CRC, suffix)", lambda: fd.png_frame_batch(files, f_off0, ol, height, width, depth, colour)),
    ("encoder, streams at aligned addresses", lambda: fd.png_filter_deflate_ultrafast_batch(pixels, p_off, chosen, t_off, enc2, o_off, rb, bpp)),
    ("encoder, streams at aligned + 41", lambda: fd.png_filter_deflate_ultrafast_batch(pixels, p_off, chosen, t_off, enc2, o_off41, rb, bpp)),
)
ts, _ = timing.interleaved(variants, 9, calls=5)
for name, _ in variants:
    show(name, ts[name])

file_len, st, _ = fd.png_encode_files_batch(pixels, p_off, files, f_off0, width, depth, colour)
info = fd.png_scan_files_batch(files, f_off0, file_len); torch.cuda.synchronize()
assert int(info[:, 0].abs().sum()) == 0
comp_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
torch.cumsum(info[:, 4].to(torch.int64), 0, out=comp_off[1:])
comp = torch.empty(int(comp_off[n]), dtype=torch.uint8, device=dev)
pix2 = torch.empty_like(pixels)
variants = (
    ("scan of %d files, CRCs verified" % n, lambda: fd.png_scan_files_batch(files, f_off0, file_len, info=info)),
    ("scan, FDH_PNG_FLAG_IGNORE_CRC", lambda: fd.png_scan_files_batch(files, f_off0, file_len, info=info, flags=fd.PNG_FLAG_IGNORE_CRC)),
    ("gather of the IDAT bodies", lambda: fd.png_gather_idat_batch(files, f_off0, info, comp, comp_off, width, depth, colour)),
    ("inflate_png_batch of the gathered streams", lambda: fd.inflate_png_batch(comp, comp_off, filt, r_off, pix2, p_off, rb, bpp)),
)
ts, _ = timing.interleaved(variants, 9, calls=5)
for name, _ in variants:
    show(name, ts[name], stream_bytes if "scan of" in name or "gather" in name else None)
print("files -> pixels give the source back: %s" % bool(torch.equal(pix2, pixels)))
