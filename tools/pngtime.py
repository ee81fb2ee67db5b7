import os, sys, torch
sys.path.insert(0, os.getcwd())
import fdeflate_amd as fd
from fdeflate_amd import synth
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


def once(f, calls=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


assert int(choose().abs().sum()) == 0
variants = (("choose", choose), ("encode", encode_chosen), ("choose + encode", choose_and_encode))
for _, f in variants:
    f(); f(); torch.cuda.synchronize()
times = {name: [] for name, _ in variants}
for _ in range(9):
    for name, f in variants:
        times[name].append(once(f))
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
