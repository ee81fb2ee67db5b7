"""Randomised parity soak on the GPU box (not collected by pytest):
    python tests/soak_gpu.py <first seed> <end seed>
General encoder (level 1 / RLE) and the PNG kernels against the oracle on random shapes and
contents, with guard bytes; several images per wavefront for the PNG pipeline; zlib / ultra-fast streams whole,
cut and damaged; cut streams' partial lengths; the resumable batch (FDH_SOAK_ONLY=resume: the last two only; =enc: the general
encoder only); the streaming object
at the reference's footprint (FDH_SOAK_ONLY=stream); random streams of tests/deflate_gen.py, which neither zlib nor the
encoders write (FDH_SOAK_ONLY=foreign)."""
import os, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import fdeflate_amd as fd
import oracle_binding as ob
import streams

def enc_round(seed):
    r = np.random.default_rng(seed)
    raws = []
    for k in range(96):
        kind = int(r.integers(0, 6))
        n = int(r.integers(0, 200000 if k % 17 == 0 else 20000))
        if kind == 0: a = r.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1: a = r.integers(0, int(r.integers(1, 8)), n, dtype=np.uint8)
        elif kind == 2: a = np.repeat(r.integers(0, 256, n // 7 + 1, dtype=np.uint8), 7)[:n]
        elif kind == 3:
            base = r.integers(0, 256, max(1, n // 50), dtype=np.uint8); a = np.tile(base, 60)[:n]
        elif kind == 4:
            a = r.integers(0, 256, n, dtype=np.uint8); a[r.random(n) < 0.8] = 0
        else:
            a = (np.cumsum(r.integers(-2, 3, n)) & 0xFF).astype(np.uint8)
        raws.append(a.tobytes())
    buf, in_off = streams.pack_exact(raws)
    caps = [fd.compress_bound(len(x)) + 3 for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64); out_off[1:] = np.cumsum(caps)
    d_in = torch.from_numpy(buf).cuda(); d_io = torch.from_numpy(in_off.astype(np.int64)).cuda(); d_oo = torch.from_numpy(out_off).cuda()
    for mode, enc in ((fd.MODE_LEVEL1, ob.compress_level1), (fd.MODE_RLE, ob.compress_rle)):
        d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        ln = fd.deflate_general_batch(d_in, d_io, d_out, d_oo, mode).cpu().numpy().view(np.uint32)
        h = d_out.cpu().numpy()
        for i, raw in enumerate(raws):
            exp = enc(raw)
            got = h[out_off[i]:out_off[i] + int(ln[i])].tobytes()
            assert got == exp, (seed, mode, i, len(raw))
            assert np.all(h[out_off[i] + int(ln[i]):out_off[i + 1]] == 0x5A)

def png_round(seed):
    r = np.random.default_rng(seed)
    bpp = int(r.choice([1, 2, 3, 4, 6, 8]))
    row_bytes = bpp * int(r.integers(1, 4300 // bpp + 1))   # up to ~4300 bytes for every bpp: both sides of the 4096-byte gate of the pipeline
    pixs, types = [], []
    for k in range(int(r.integers(1, 60))):
        rows = int(r.integers(0, 150))
        pixs.append(bytes(r.integers(0, 256 if k % 3 else 3, row_bytes * rows, dtype=np.uint8)))
        types.append(bytes(r.integers(0, 5, rows, dtype=np.uint8)))
    filts = [ob.png_filter(p, row_bytes, bpp, t)[1] for p, t in zip(pixs, types)]
    pbuf, poff = streams.pack_exact(pixs); tbuf, toff = streams.pack_exact(types); fbuf, foff = streams.pack_exact(filts)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for pw in ("1", "2", "5", "8"):
        os.environ["FDH_PNG_IMAGES_PER_WAVE"] = pw
        d_f = torch.full((int(foff[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        st = fd.png_filter_batch(d(pbuf), d(poff.astype(np.int64)), d(tbuf), d(toff.astype(np.int64)), d_f, d(foff.astype(np.int64)), row_bytes, bpp)
        h = d_f.cpu().numpy(); nf = int(foff[-1])
        assert int(st.abs().sum()) == 0 and h[:nf].tobytes() == fbuf[:nf].tobytes() and np.all(h[nf:] == 0xEE), (seed, pw, "filter")
        d_o = torch.full((int(poff[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
        st = fd.png_unfilter_batch(d(fbuf), d(foff.astype(np.int64)), d_o, d(poff.astype(np.int64)), row_bytes, bpp)
        h = d_o.cpu().numpy(); npx = int(poff[-1])
        assert int(st.abs().sum()) == 0 and h[:npx].tobytes() == pbuf[:npx].tobytes() and np.all(h[npx:] == 0xEE), (seed, pw, "unfilter", bpp, row_bytes)

    # the filters fused into the ultra-fast encoder: pixel rows in, the oracle's encoding of the oracle's filtered image out
    bound = [int(fd.ultrafast_bound(len(f))) + 16 for f in filts]
    ooff = np.zeros(len(filts) + 1, dtype=np.int64); ooff[1:] = np.cumsum(bound)
    d_z = torch.full((int(ooff[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
    ol, st = fd.png_filter_deflate_ultrafast_batch(d(pbuf) if pbuf.size else torch.zeros(1, dtype=torch.uint8, device="cuda"), d(poff.astype(np.int64)),
                                                   d(tbuf) if tbuf.size else torch.zeros(1, dtype=torch.uint8, device="cuda"), d(toff.astype(np.int64)),
                                                   d_z, d(ooff), row_bytes, bpp)
    torch.cuda.synchronize()
    h, oll = d_z.cpu().numpy(), ol.cpu().tolist()
    assert int(st.abs().sum()) == 0, (seed, "fused status")
    for i, f in enumerate(filts):
        assert h[ooff[i]:ooff[i] + oll[i]].tobytes() == ob.compress_ultra_fast(f), (seed, "fused", i, bpp, row_bytes, len(f))
        assert np.all(h[ooff[i] + oll[i]:ooff[i + 1]] == 0xEE), (seed, "fused guard", i)

def dec_round(seed):
    """zlib streams of every level / strategy over mixed data, whole, truncated and with a flipped
    byte, in exact / loose / short slots: status, length, bytes and checksum against the oracle."""
    r = np.random.default_rng(seed)
    comps, caps = [], []
    for k in range(64):
        n = int(r.integers(0, 60000))
        kind = int(r.integers(0, 4))
        if kind == 0: a = r.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1: a = r.integers(0, int(r.integers(1, 6)), n, dtype=np.uint8)
        elif kind == 2: a = np.tile(r.integers(0, 256, max(1, n // 40), dtype=np.uint8), 50)[:n]
        else: a = (np.cumsum(r.integers(-1, 2, n)) & 0xFF).astype(np.uint8)
        co = zlib.compressobj(int(r.integers(0, 10)), zlib.DEFLATED, 15, int(r.integers(1, 10)), int(r.choice([0, 1, 2, 3, 4])))
        c = co.compress(a.tobytes()) + co.flush()
        mut = int(r.integers(0, 6))
        if mut == 1 and len(c) > 8: c = c[:int(r.integers(2, len(c)))]
        if mut == 2 and len(c) > 8:
            b = bytearray(c); b[int(r.integers(2, len(c)))] ^= 1 << int(r.integers(0, 8)); c = bytes(b)
        comps.append(c)
        caps.append(int(r.choice([n, n + 100, max(0, n - int(r.integers(1, 50))), n])))
    cbuf, coff = streams.pack_exact(comps)
    ooff = np.zeros(len(comps) + 1, dtype=np.int64); ooff[1:] = np.cumsum([c + 16 for c in caps])
    slot = np.zeros(len(comps) + 1, dtype=np.int64)
    # slots of exactly `cap` bytes, 16 guard bytes behind each
    starts = ooff[:-1]
    d_out = torch.full((int(ooff[-1]) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    # the API takes one offsets array: build it so that slot i = [starts[i], starts[i] + caps[i])
    # by decoding stream by stream groups is overkill -- use per-stream calls through a packed layout instead
    o2 = np.zeros(2 * len(comps) + 1, dtype=np.int64)
    i2 = np.zeros(2 * len(comps) + 1, dtype=np.int64)
    for i in range(len(comps)):
        o2[2 * i] = starts[i]; o2[2 * i + 1] = starts[i] + caps[i]
        i2[2 * i] = coff[i]; i2[2 * i + 1] = coff[i + 1]
    o2[-1] = ooff[-1]; i2[-1] = coff[-1]
    # odd entries are zero-length inputs (BadZlibHeader / InsufficientInput slots of 16 guard bytes): ignored below
    ol, st, ad = fd.inflate_batch(torch.from_numpy(cbuf).cuda(), torch.from_numpy(i2).cuda(), d_out, torch.from_numpy(o2).cuda())
    ol, st, ad, h = ol.cpu().numpy().view(np.uint32), st.cpu().numpy(), ad.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    for i, c in enumerate(comps):
        est, eout, ead = ob.decompress_bounded(c, caps[i])
        assert int(st[2 * i]) == est, (seed, i, int(st[2 * i]), est)
        if est == 0:
            assert int(ol[2 * i]) == len(eout) and h[starts[i]:starts[i] + len(eout)].tobytes() == eout and int(ad[2 * i]) == ead, (seed, i)
        assert np.all(h[starts[i] + caps[i]:starts[i] + caps[i] + 16] == 0xA5), (seed, i, "guard")


def uf_round(seed):
    """Ultra-fast-format streams (what the interval decoder takes) over mixed data -- noise, long
    zero stretches, short runs, rows of repeated bytes, sizes from 0 to ~400 KB -- whole, truncated,
    with a flipped bit, with a wrong checksum, in exact / loose / short slots: the whole pipeline,
    the pipeline without the interval kernel and the interval kernel alone against the oracle."""
    r = np.random.default_rng(seed)
    comps, caps = [], []
    for k in range(48):
        big = k % 11 == 0
        n = int(r.integers(0, 400000 if big else 70000))
        kind = int(r.integers(0, 6))
        if kind == 0: a = r.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            a = r.integers(0, 256, n, dtype=np.uint8); a[r.random(n) < float(r.choice([0.3, 0.8, 0.97]))] = 0
        elif kind == 2:
            a = np.zeros(n, dtype=np.uint8)
            for _ in range(int(r.integers(0, 12))):
                if n: a[int(r.integers(0, n))] = int(r.integers(1, 256))
        elif kind == 3:
            a = r.integers(0, 256, n, dtype=np.uint8)
            for _ in range(int(r.integers(1, 20))):
                if n:
                    lo = int(r.integers(0, n)); a[lo:lo + int(r.integers(1, 3000))] = 0
        elif kind == 4: a = np.repeat(r.integers(0, 4, n // 5 + 1, dtype=np.uint8), 5)[:n]
        else: a = (r.integers(0, 256, n, dtype=np.uint8) & int(r.choice([1, 3, 15, 255]))).astype(np.uint8)
        c = ob.compress_ultra_fast(a.tobytes())
        mut = int(r.integers(0, 8))
        if mut == 1 and len(c) > 60: c = c[:int(r.integers(54, len(c)))]
        if mut == 2 and len(c) > 60:
            b = bytearray(c); b[int(r.integers(53, len(c)))] ^= 1 << int(r.integers(0, 8)); c = bytes(b)
        if mut == 3:
            b = bytearray(c); b[-1] ^= 0x40; c = bytes(b)
        comps.append(c)
        caps.append(int(r.choice([n, n, n + 100, n + 7, max(0, n - int(r.integers(1, 300)))])))
    cbuf, coff = streams.pack_exact(comps)
    ooff = np.zeros(len(comps) + 1, dtype=np.int64); ooff[1:] = np.cumsum([c + 16 for c in caps])
    starts = ooff[:-1]
    o2 = np.zeros(2 * len(comps) + 1, dtype=np.int64)
    i2 = np.zeros(2 * len(comps) + 1, dtype=np.int64)
    for i in range(len(comps)):
        o2[2 * i] = starts[i]; o2[2 * i + 1] = starts[i] + caps[i]
        i2[2 * i] = coff[i]; i2[2 * i + 1] = coff[i + 1]
    o2[-1] = ooff[-1]; i2[-1] = coff[-1]
    exp = [ob.decompress_bounded(c, caps[i]) for i, c in enumerate(comps)]
    d_c, d_i, d_o = torch.from_numpy(cbuf).cuda(), torch.from_numpy(i2).cuda(), torch.from_numpy(o2).cuda()
    only = (fd.api.FLAG_INTERVALS_ONLY, fd.api.FLAG_INTERVALS_ONLY | fd.api.FLAG_NO_LANDING, fd.api.FLAG_LANDING_ONLY,
            fd.api.FLAG_LANDING_ONLY | fd.api.FLAG_NO_LEAN_WRITE)
    for flags in (0, fd.api.FLAG_NO_INTERVALS, fd.api.FLAG_NO_LANDING, fd.api.FLAG_NO_LEAN_WRITE) + only:
        d_out = torch.full((int(ooff[-1]) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        ol, st, ad = fd.inflate_batch(d_c, d_i, d_out, d_o, flags=flags)
        ol, st, ad, h = ol.cpu().numpy().view(np.uint32), st.cpu().numpy(), ad.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
        for i, c in enumerate(comps):
            est, eout, ead = exp[i]
            got = int(st[2 * i])
            assert np.all(h[starts[i] + caps[i]:starts[i] + caps[i] + 16] == 0xA5), (seed, flags, i, "guard")
            if flags in only and got != 0:
                continue  # left to the kernels behind it (not run here): only what it finishes is checked
            assert got == est, (seed, flags, i, got, est)
            if est == 0:
                assert int(ol[2 * i]) == len(eout) and h[starts[i]:starts[i] + len(eout)].tobytes() == eout and int(ad[2 * i]) == ead, (seed, flags, i)


def order_round(seed):
    """A batch large enough for the interval kernel's hand-out order (several streams per persistent
    wavefront): ~17 000 ultra-fast streams of random lengths, a random share of them long, a few
    replaced by zlib streams; encoded on the GPU (bit-exact with the oracle elsewhere), decoded,
    compared with the raw bytes, checksums against the trailers."""
    r = np.random.default_rng(seed)
    n = 16384 + int(r.integers(0, 2000))
    lens = r.integers(0, int(r.choice([300, 2000, 6000])), n)
    k = int(r.choice([4, 8, 32]))
    lens[::k] = r.integers(8000, 50000, len(lens[::k]))
    total = int(lens.sum())
    raw_h = r.integers(0, 256, total, dtype=np.uint8)
    raw_h[r.random(total) < float(r.choice([0.2, 0.7, 0.95]))] = 0
    r_off_h = np.zeros(n + 1, dtype=np.int64); r_off_h[1:] = np.cumsum(lens)
    bounds = ((np.array([fd.ultrafast_bound(int(x)) for x in lens], dtype=np.int64) + 15) & ~15)
    c_off_h = np.zeros(n + 1, dtype=np.int64); c_off_h[1:] = np.cumsum(bounds)
    raw, r_off, c_off = torch.from_numpy(raw_h).cuda(), torch.from_numpy(r_off_h).cuda(), torch.from_numpy(c_off_h).cuda()
    comp = torch.zeros(int(c_off_h[-1]), dtype=torch.uint8, device="cuda")
    clen = fd.deflate_ultrafast_batch(raw, r_off, comp, c_off).cpu().numpy().astype(np.int64)
    comp_h = comp.cpu().numpy()
    for i in r.integers(0, n, 12):
        z = zlib.compress(raw_h[r_off_h[i]:r_off_h[i + 1]].tobytes(), int(r.integers(1, 10)))
        if len(z) <= bounds[i]:
            comp_h[c_off_h[i]:c_off_h[i] + bounds[i]] = 0
            comp_h[c_off_h[i]:c_off_h[i] + len(z)] = np.frombuffer(z, dtype=np.uint8)
            clen[i] = len(z)
    comp = torch.from_numpy(comp_h).cuda()
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ol, st, ad = fd.inflate_batch(comp, c_off, out, r_off)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0, seed
    assert torch.equal(ol.to(torch.int64), torch.from_numpy(lens).cuda()), seed
    assert torch.equal(out[:total], raw) and bool((out[total:] == 0xA5).all()), seed
    adh = ad.cpu().numpy().view(np.uint32)
    for i in r.integers(0, n, 64):
        t = comp_h[c_off_h[i] + clen[i] - 4:c_off_h[i] + clen[i]]
        assert int(adh[i]) == int.from_bytes(t.tobytes(), "big"), (seed, i)


def _rand_buffer(r, n):
    kind = int(r.integers(0, 6))
    if kind == 0: return r.integers(0, 256, n, dtype=np.uint8)
    if kind == 1: return r.integers(0, int(r.integers(1, 8)), n, dtype=np.uint8)
    if kind == 2: return np.tile(r.integers(0, 256, max(1, n // 40), dtype=np.uint8), 50)[:n]
    if kind == 3:
        a = r.integers(0, 256, n, dtype=np.uint8); a[r.random(n) < 0.8] = 0; return a
    if kind == 4: return (r.integers(-3, 4, n) & 0xFF).astype(np.uint8)     # small residuals: short codes, pairs of literals
    return (np.cumsum(r.integers(-2, 3, n)) & 0xFF).astype(np.uint8)


def _rand_stream(r, n):
    a = _rand_buffer(r, n).tobytes()
    if int(r.integers(0, 3)) == 0:
        return ob.compress_ultra_fast(a), a
    co = zlib.compressobj(int(r.integers(0, 10)), zlib.DEFLATED, 15, int(r.integers(1, 10)), int(r.choice([0, 1, 2, 3, 4])))
    return co.compress(a) + co.flush(), a


def cut_round(seed):
    """Streams of both formats cut at random places: InsufficientInput with the length and the bytes the
    oracle's streaming decoder had produced from that prefix (what the check points / the step tracking of the
    tile decoders are for), with and without check points."""
    import gpu_harness
    r = np.random.default_rng(seed)
    blobs, exp = [], []
    for k in range(48):
        c, a = _rand_stream(r, int(r.integers(200, 90000)))
        for cut in sorted(set(int(x) for x in r.integers(3, max(4, len(c)), 6))):
            d = ob.Decompressor()
            out = np.zeros(len(a) + 64, dtype=np.uint8)
            st, cons, p = d.read(c[:cut], out, 0)
            if st == 0 and not d.is_done():
                blobs.append(c[:cut]); exp.append(out[:p].tobytes())
    caps = [len(e) + 300 for e in exp]
    for flags in (0, 0x4000, 0x1000):
        st, ln, ad, outs, ok = gpu_harness.gpu_inflate(blobs, caps, flags)
        assert ok, (seed, "guard")
        for i, e in enumerate(exp):
            assert int(st[i]) == 2 and int(ln[i]) == len(e) and outs[i][:len(e)].tobytes() == e, (seed, flags, i, int(st[i]), int(ln[i]), len(e))


def resume_round(seed):
    """fdh_inflate_batch_resumable: random streams, the input and the slot growing in random steps, some of them
    damaged: the last call's status, length, checksum and bytes are those of one call on the whole stream."""
    import gpu_harness
    r = np.random.default_rng(seed)
    comps, caps = [], []
    for k in range(24):
        c, a = _rand_stream(r, int(r.integers(1, 120000)))
        mut = int(r.integers(0, 8))
        if mut == 1 and len(c) > 8:
            b = bytearray(c); b[int(r.integers(2, len(c)))] ^= 1 << int(r.integers(0, 8)); c = bytes(b)
        if mut == 2 and len(c) > 8: c = c[:int(r.integers(2, len(c)))]
        comps.append(c)
        caps.append(max(1, len(a) + int(r.choice([0, 0, 50, -int(r.integers(1, 40))]))))
    steps = int(r.integers(2, 7))
    in_cuts = [sorted(int(x) for x in r.integers(1, len(c) + 1, steps - 1)) + [len(c)] for c in comps]
    out_cuts = [sorted(int(x) for x in r.integers(1, cap + 1, steps - 1)) + [cap] for cap in caps]
    (ln, st, ad), outs, guards, _ = gpu_harness.drive_resumable(fd, comps, in_cuts, out_cuts)
    assert guards, (seed, "guard")
    for i, c in enumerate(comps):
        est, eout, ead = ob.decompress_bounded(c, caps[i])
        assert int(st[i]) == est, (seed, i, int(st[i]), est)
        if est in (0, 17):
            assert int(ln[i]) == len(eout) and outs[i][:len(eout)].tobytes() == eout, (seed, i, int(ln[i]), len(eout))
        if est == 0:
            assert int(ad[i]) == ead, (seed, i)


def stream_round(seed):
    """The streaming Decompressor at the reference's footprint (round 5): streams of 0.2-2 MB in both formats, whole,
    cut short or with a flipped bit, the input offered in random pieces (what is not consumed is offered again), the
    output drained through a random window with 32 KiB of history in front, as png does.  The bytes delivered are the
    oracle's (all of them for a whole stream; for a cut one what the oracle's streaming decoder produces from the same
    prefix; for a damaged one the bytes in front of the damage, to within two windows, and the oracle's error), and the device memory stays
    under 1.5 MiB + three windows (stored blocks are taken up at their headers: 64 KiB at a time)."""
    r = np.random.default_rng(seed)
    for k in range(3):
        c, a = _rand_stream(r, int(r.integers(200_000, 2_000_000)))
        mut = int(r.integers(0, 4))
        if mut == 1:
            b = bytearray(c); b[int(r.integers(len(c) // 4, len(c)))] ^= 1 << int(r.integers(0, 8)); c = bytes(b)
        if mut == 2:
            c = c[:int(r.integers(len(c) // 4, len(c)))]
        est, eout, _ = ob.decompress_bounded(c, len(a) + 4096)            # the one-shot classification
        _, sout = ob.decompress_by_chunks(c, 0, len(a) + 4096)            # what a streaming decoder delivers from it
        window = int(r.choice([1024, 4096, 16384, 65536]))
        piece = int(r.choice([1, 3, 17, 64, 200])) * 1024
        d = fd.Decompressor()
        buf = bytearray(32768 + window)
        got = bytearray()
        pos = kpos = calls = idle = 0
        status = 0
        while not d.is_done():
            calls += 1
            assert calls < 200_000, (seed, k)
            try:
                cns, p = d.read(c[kpos:kpos + piece], buf, pos)
            except fd.DecompressionError as e:
                status = e.status
                break
            kpos += cns
            got += buf[pos:pos + p]
            pos += p
            if pos > 32768:
                buf[:32768] = buf[pos - 32768:pos]
                pos = 32768
            idle = idle + 1 if (p == 0 and cns == 0 and kpos >= len(c)) else 0
            if idle >= 2:
                break                       # the input is used up and an empty read produced nothing: cut short
            assert os.environ.get("FDH_STREAM_NO_RESUME") or d.device_bytes() <= (3 << 19) + 3 * window, (seed, k, d.device_bytes(), window)
        if est == 0:
            assert status == 0 and d.is_done() and bytes(got) == a, (seed, k, status, len(got), len(a))
        elif est == 2:                      # InsufficientInput: everything the prefix holds, and not done
            assert status == 0 and not d.is_done() and bytes(got) == sout, (seed, k, status, len(got), len(sout))
        elif est == 17:                     # (the damage made the stream longer than the one-shot slot: nothing to compare with)
            pout = ob.decompress_by_chunks(c, max(256, len(c) // 4000), len(a) + 4096)[1]
            m = min(len(got), len(pout))
            assert bytes(got[:m]) == pout[:m], (seed, k)
        else:
            assert status == est, (seed, k, status, est)
            # (the bytes in front of the damage, to within the call that fails -- here and there: the oracle's streaming
            #  decoder fed small pieces delivers everything up to its failing call)
            _, pout = ob.decompress_by_chunks(c, max(256, len(c) // 4000), len(a) + 4096)
            m = min(len(got), len(pout))
            assert bytes(got[:m]) == pout[:m] and len(got) + 2 * window + 600 >= len(pout), (seed, k, len(got), len(pout), window)


def foreign_round(seed):
    """Random deflate_gen streams of both kinds -- random complete codes up to 15 bits, blocks of every type, matches of
    every length and distance; random runs of every byte cut under a random policy behind the ultra-fast prefix --
    checked three ways on the CPU, then through the whole pipeline and each kernel alone: what is reported is the
    oracle's status, length, bytes and Adler-32, the guards stay, and only a single-kernel run may leave a stream."""
    import deflate_gen, gpu_harness
    r = np.random.default_rng(seed)
    comps, raws, kinds = [], [], []
    for k in range(48):
        uf = k % 2 == 0
        c, a = deflate_gen.random_uf(r) if uf else deflate_gen.random_general(r)
        est, eout, ead = ob.decompress_bounded(c, len(a))
        assert zlib.decompress(c) == a and est == 0 and eout == a and ead == zlib.adler32(a), (seed, k, "the references disagree")
        comps.append(c); raws.append(a); kinds.append(uf)
    caps = [len(a) + int(r.choice([0, 0, 16, 100])) for a in raws]
    gpu_harness.assert_inflate_parity(["s%d_%d" % (seed, k) for k in range(len(comps))], comps, caps)
    only_uf = (fd.api.FLAG_LANDING_ONLY, fd.api.FLAG_LANDING_ONLY | fd.api.FLAG_NO_LEAN_WRITE, fd.api.FLAG_INTERVALS_ONLY,
               fd.api.FLAG_NO_INTERVALS | fd.api.FLAG_FIRST_ONLY, fd.api.FLAG_FIRST_ONLY)
    for flags in only_uf + (0x2000,):
        st, ln, ad, outs, ok = gpu_harness.gpu_inflate(comps, caps, flags)
        assert ok, (seed, flags, "guard")
        for i, a in enumerate(raws):
            if int(st[i]) >= 0xFFFFFFFD:
                continue  # left to the kernels behind it (not run here)
            assert int(st[i]) == 0 and int(ln[i]) == len(a) and outs[i][:len(a)].tobytes() == a and int(ad[i]) == zlib.adler32(a), (seed, flags, i)


ONLY = os.environ.get("FDH_SOAK_ONLY", "")
for s in range(int(sys.argv[1]), int(sys.argv[2])):
    if ONLY == "stream":
        stream_round(8000 + s)
        print("seed", s, "ok", flush=True)
        continue
    if ONLY == "png":
        png_round(12000 + s)
        print("seed", s, "ok", flush=True)
        continue
    if ONLY == "enc":  # the general encoder alone (new seeds: the default rounds use 1000 + s)
        enc_round(9000 + s)
        print("seed", s, "ok", flush=True)
        continue
    if ONLY == "foreign":
        foreign_round(13000 + s)
        print("seed", s, "ok", flush=True)
        continue
    if ONLY == "resume":
        cut_round(6000 + s); resume_round(7000 + s)
        print("seed", s, "ok", flush=True)
        continue
    if ONLY not in ("uf", "order"):
        enc_round(1000 + s); png_round(2000 + s); dec_round(3000 + s); cut_round(6000 + s); resume_round(7000 + s); stream_round(8000 + s)
    if ONLY != "order":
        uf_round(4000 + s)
    if s % 8 == 0 or ONLY == "order":
        order_round(5000 + s)
    print("seed", s, "ok", flush=True)
print("SOAK OK")
