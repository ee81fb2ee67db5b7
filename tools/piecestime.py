"""Times long inputs in pieces (fdeflate_amd.pieces) against the whole-stream route, and writes what it prints to
profiles/pieces_time.txt as well.

    python tools/piecestime.py [--pictures 1,16] [--side 1024] [--levels 1,3] [--rounds 3] [--out profiles/pieces_time.txt]
    python tools/piecestime.py --cpu-sizes        (the size cost from the models of tests/, no device)

Device events (tools/timing.py's `once`), one warm-up call per variant and picture count (two of the piece route),
then `rounds` rounds in which the variants ALTERNATE; per variant: median [minimum .. maximum] over the rounds.  A whole-stream call on a long input
runs for seconds, so a round is ONE call of it; the piece route's rounds fill a fifth of a second.
  (1) png_encode_mixed_rgba_files_level_batch -- one stream per picture -- against
      png_encode_mixed_rgba_files_level_pieces_batch at piece sizes of 32, 64, 128 and 256 KiB, on 1 and 16 pictures of
      side x side RGBA8 made of the bench's synthetic rows (forced to (8, 6): side * (4 side + 1) bytes of filtered
      rows each), at every level of --levels; the files' sizes by both routes; every file of the piece route decoded
      back on the device.
  (2) level 6: the whole-stream route on ONE call at 256 x 256 (a 4 MiB lane would run for tens of seconds), the piece
      route there and at side x side.
  (3) the stitch kernels alone on the bench shape, 8 192 inputs of 64 KiB with one piece each: what they cost an input
      that did not need splitting, in ms and TB/s of bytes read + written.
"""
import argparse
import builtins
import math
import os
import sys

sys.path.insert(0, os.getcwd())

ap = argparse.ArgumentParser()
ap.add_argument("--pictures", default="1,16")
ap.add_argument("--side", type=int, default=1024)
ap.add_argument("--levels", default="1,3")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cpu-sizes", action="store_true")
ap.add_argument("--out", default=os.path.join("profiles", "pieces_time.txt"))
args = ap.parse_args()
PIECE_KIB = (32, 64, 128, 256)

if args.cpu_sizes:
    # stitched bytes against whole-stream bytes from the models: 256 KiB of the bench's rows, pieces of 16 .. 128 KiB
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import pieces_model as pm
    from fdeflate_amd import synth
    data = b"".join(synth.gen_stream_np(i, 65536).tobytes() for i in range(4))
    print("the models on %d bytes of the bench's synthetic rows: stitched bytes / whole-stream bytes" % len(data))
    for level in (1, 3, 6):
        whole = len(pm.compress(data, level, 1 << 30))
        print("  level %d: whole %d bytes; " % (level, whole) +
              ", ".join("%d KiB pieces %.4f" % (k, len(pm.compress(data, level, k << 10)) / whole) for k in (16, 32, 64, 128)))
    sys.exit(0)

import torch  # noqa: E402

import fdeflate_amd as fd  # noqa: E402
from fdeflate_amd import pieces, png_levels, synth  # noqa: E402
import timing  # noqa: E402
from timing import arange_off  # noqa: E402

dev = "cuda"
log = open(args.out, "w")
builtins_print = builtins.print


def print(*a, **k):  # noqa: A001 (everything goes to the file as well)
    builtins_print(*a, **k)
    builtins_print(*a, **dict(k, file=log))
    log.flush()
    sys.stdout.flush()


def rounds_of(variants, rounds, window_ms=200.0):
    """[(name, f, one call per round?)] -> {name: (median, minimum, maximum)}: the variants in turn, every one warm from
    its caller; one more call of those that take several per round says how many."""
    calls = {}
    for name, f, single in variants:
        calls[name] = 1 if single else max(1, int(math.ceil(window_ms / max(timing.once(f, 1), 1e-3))))
    ts = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, f, _ in variants:
            ts[name].append(timing.once(f, calls[name]))
    stats = {}
    for name, _, _ in variants:
        t = sorted(ts[name])
        stats[name] = (t[len(t) // 2], t[0], t[-1])
        print("    %-58s median %10.3f ms [%10.3f .. %10.3f] over %d rounds of %d calls" % (name, t[len(t) // 2], t[0], t[-1], len(t), calls[name]))
    return stats


def pictures_of(count, side):
    """`count` RGBA8 pictures of side x side: the bench's synthetic RGB rows (341 pixels, 64 to a stream) unfiltered, three
    streams side by side and side / 64 of them down, the last column repeated, alpha 255."""
    L, rows = 65536, 65536 // synth.ROW_BYTES
    width = (synth.ROW_BYTES - 1) // 3
    across, down = -(-side // width), -(-side // rows)
    n = count * across * down
    rb, bpp = fd.png_geometry(width, 8, 2)
    filtered = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
    pix = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
    fd.png_unfilter_batch(filtered, arange_off(n, L), pix, arange_off(n, rows * rb), rb, bpp)
    rgb = pix.view(count, down, across, rows, width, 3).permute(0, 1, 3, 2, 4, 5).reshape(count, down * rows, across * width, 3)
    rgb = rgb[:, :side, :side] if across * width >= side else torch.cat((rgb, rgb[:, :, -1:].expand(-1, -1, side - across * width, -1)), 2)[:, :side]
    rgba = torch.full((count, side, side, 4), 255, dtype=torch.uint8, device=dev)
    rgba[..., :3] = rgb[:, :side, :side]
    return rgba.reshape(-1).contiguous(), arange_off(count, side * side * 4)


def compare(count, side, level, piece_kib, whole_rounds):
    rgba, r_off = pictures_of(count, side)
    w_t = torch.full((count,), side, dtype=torch.int32, device=dev)
    filtered = side * (4 * side + 1)
    whole = lambda: png_levels.png_encode_mixed_rgba_files_level_batch(rgba, r_off, w_t, w_t, level, pairs=(8, 6))
    variants = [("whole streams (png_levels), level %d" % level, whole, True)] if whole_rounds else []
    for k in piece_kib:
        variants.append(("pieces of %3d KiB, level %d" % (k, level),
                         (lambda k: lambda: pieces.png_encode_mixed_rgba_files_level_pieces_batch(rgba, r_off, w_t, w_t, level, pairs=(8, 6),
                                                                                                 piece_bytes=k << 10))(k), False))
    print("  %d picture(s) of %d x %d RGBA8 as (8, 6), %d bytes of filtered rows each, level %d" % (count, side, side, filtered, level))
    # sizes and the round trip first (these calls are the warm-up of the code objects)
    sizes = {}
    for name, f, _ in variants:
        file, f_off, f_len, st, _ = f()
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0, name
        sizes[name] = int(f_len.to(torch.int64).sum())
        if "pieces" in name:
            back, _, _, status, png_status = fd.png_decode_mixed_files_rgba_batch(file, f_off, file_len=f_len)
            torch.cuda.synchronize()
            assert int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0 and torch.equal(back[:rgba.numel()], rgba), name
    stats = rounds_of(variants, args.rounds if whole_rounds != 1 else 1)
    base = variants[0][0]
    for name, _, _ in variants[1:]:
        line = "    %s: files %.4f of the first variant's bytes (%d / %d)" % (name, sizes[name] / sizes[base], sizes[name], sizes[base])
        if whole_rounds:
            line += "; %.1f x faster (medians)" % (stats[base][0] / stats[name][0])
        print(line)
    if whole_rounds:
        m = stats[base][0]
        print("    whole streams: %.1f KiB/s per picture" % (filtered / 1024 / (m / 1e3)))
    print("    the piece route's files decode back to the pictures on the device: True")


print("device: %s" % torch.cuda.get_device_name(0))
levels_ = [int(v) for v in args.levels.split(",") if v]
print("(1) whole streams against pieces")
for level in levels_:
    for count in [int(v) for v in args.pictures.split(",") if v]:
        compare(count, args.side, level, PIECE_KIB, whole_rounds=args.rounds)
print("(2) level 6: whole streams at 256 x 256 only, ONE timed call; the piece route there and at %d x %d" % (args.side, args.side))
compare(1, 256, 6, (32, 64), whole_rounds=1)
for count in (1, 16):
    compare(count, args.side, 6, PIECE_KIB, whole_rounds=0)

print("(3) the stitch kernels alone: 8 192 inputs of 64 KiB, one piece each (level 1 pieces of the bench's rows)")
n, L = 8192, 65536
raw = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)
p_off = arange_off(n, L)
slot = (fd.compress_bound(L) + 15) & ~15
slots, s_off = torch.empty(n * slot, dtype=torch.uint8, device=dev), arange_off(n, slot)
last = torch.ones(n, dtype=torch.uint8, device=dev)
p_len, p_adler = pieces.deflate_level_pieces_raw_batch(raw, p_off, last, slots, s_off, 1)
first = torch.arange(n + 1, dtype=torch.int64, device=dev)
out, o_off, o_len = torch.empty(n * slot + 41, dtype=torch.uint8, device=dev), arange_off(n, slot, 41), torch.empty(n, dtype=torch.int32, device=dev)
adler = p_adler.clone()


def stitch():
    adler.copy_(p_adler)                        # (the call leaves the pieces' places there)
    pieces.deflate_stitch_batch(slots, s_off, p_len, adler, p_off, first, out, o_off, out_len=o_len)


stitch()
torch.cuda.synchronize()
moved = int(p_len.to(torch.int64).sum())
assert bool((o_len == p_len + 6).all())
stats = rounds_of((("stitch (plan + copy) behind a 32 KiB copy of the checksums", stitch, False),
                   ("the copy of the checksums alone", lambda: adler.copy_(p_adler), False)), max(args.rounds, 5))
t = stats["stitch (plan + copy) behind a 32 KiB copy of the checksums"][0] - stats["the copy of the checksums alone"][0]
print("    %d piece bytes (%.1f per input), read once and written once: %.3f ms, %.3f TB/s of bytes read + written" %
      (moved, moved / n, t, 2 * moved / t / 1e9))
log.close()
