"""-m gpu: the HIP path, called through the C ABI, against the CPU oracle -- bit-exact."""
import os
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


def _norm_gpu_lit(e):
    nb, kind = e & 15, (e >> 4) & 15
    if kind == 0:
        return ("lit1", (e >> 8) & 0xFF, nb)
    if kind == 1:
        return ("lit2", (e >> 8) & 0xFF, (e >> 16) & 0xFF, nb)
    if kind == 2:
        return ("len", e >> 16, (e >> 8) & 31, nb)
    if kind == 3:
        return ("eob", nb)
    return ("long",)


def _norm_ref_lit(e):
    if e & 0x8000:
        n = (e >> 8) & 0xF
        if n == 1:
            return ("lit1", (e >> 16) & 0xFF, e & 0xFF)
        return ("lit2", (e >> 16) & 0xFF, (e >> 24) & 0xFF, e & 0xFF)
    if e & 0x2000:
        return ("long",)
    if e & 0x4000:
        return ("eob", e & 0xFF)
    return ("len", e >> 16, (e >> 8) & 0xFF, e & 0xFF)


def _norm_gpu_dist(e):
    nb, kind = e & 15, (e >> 4) & 15
    if kind == 1:
        return ("dist", e >> 16, (e >> 8) & 15, nb)
    if kind == 2:
        return ("long",)
    return ("invalid",)


def _norm_ref_dist(e):
    if e & 0x8000:
        return ("dist", e >> 16, (e >> 8) & 0xF, e & 0xFF)
    if (e >> 8) == 0:
        return ("invalid",)
    return ("long",)


def _code_length_sets(golden_constants):
    sets = []
    sets.append(("fixed", 288, [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32))
    sets.append(("ultrafast", 286, golden_constants["HUFFMAN_LENGTHS"] + [0, 0] + [1] + [0] * 31))
    sets.append(("long15", 286, streams.long_code_lengths() + [0, 0] + [1, 1] + [0] * 30))
    sets.append(("mixed_long", 286, streams.mixed_long_lengths() + [0, 0] +
                 [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15] + [0] * 16))
    sets.append(("flat_nodist", 286, streams.flat_lengths() + [0, 0] + [0] * 32))
    sets.append(("hlit257", 257, [8] * 255 + [9, 9] + [0] * 31 + [5] * 30 + [0, 0]))
    return sets


def test_device_table_builder_matches_reference_tables(harness, golden_constants):
    import fdeflate_amd as fd
    for name, hlit, cl in _code_length_sets(golden_constants):
        assert len(cl) == 320, name
        rst, rlit, rdist, reof = ob.build_decode_tables(hlit, cl)
        gst, glit, gdist, geof = fd.debug_build_tables(cl, hlit)
        assert gst == rst, (name, gst, rst)
        if rst != 0:
            continue
        assert geof == reof, (name, geof, reof)
        for i in range(4096):
            assert _norm_gpu_lit(int(glit[i])) == _norm_ref_lit(int(rlit[i])), (name, i)
        for i in range(512):
            assert _norm_gpu_dist(int(gdist[i])) == _norm_ref_dist(int(rdist[i])), (name, "dist", i)
    # golden: the fixed table is the reference constant FIXED_LITLEN_TABLE (tables.rs:142-195)
    gst, glit, gdist, _ = fd.debug_build_tables([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32, 288)
    for i in range(512):
        assert _norm_gpu_lit(int(glit[i])) == _norm_ref_lit(golden_constants["FIXED_LITLEN_TABLE"][i])
    for i in range(32):
        assert _norm_gpu_dist(int(gdist[i])) == _norm_ref_dist(golden_constants["FIXED_DIST_TABLE"][i])


def test_table_builder_error_codes(harness):
    import fdeflate_amd as fd
    flat = streams.flat_lengths()
    cases = {
        "no_eob": [8] * 256 + [0] * 32 + [1, 1] + [0] * 30,
        "incomplete": [9] + flat[1:] + [0, 0] + [1, 1] + [0] * 30,
        "over": flat[:285] + [8] + [0, 0] + [1, 1] + [0] * 30,
        "dist_incomplete": flat + [0, 0] + [2, 2, 2] + [0] * 29,
        "dist_lone2": flat + [0, 0] + [2] + [0] * 31,
        "dist_single_sym5": flat + [0, 0] + [0] * 5 + [1] + [0] * 26,
    }
    for name, cl in cases.items():
        rst = ob.build_decode_tables(286, cl)[0]
        gst = fd.debug_build_tables(cl, 286)[0]
        assert gst == rst, (name, gst, rst)


def _caps_for(raw_len):
    return sorted(set([raw_len, raw_len + 1, raw_len + 777, max(raw_len - 1, 0), raw_len // 2, 0]))


def test_valid_streams_all_block_types(harness):
    names, blobs, caps = [], [], []
    for name, comp, raw in streams.valid_streams():
        for c in _caps_for(len(raw)):
            names.append("%s@%d" % (name, c))
            blobs.append(comp)
            caps.append(c)
    harness.assert_inflate_parity(names, blobs, caps)


def test_valid_streams_every_decoder_variant(harness):
    """The same valid streams through each decoder on its own: shared-table + tiles without the
    serial re-check (8), general kernel with tiles (4|8), serial only (2).  With the re-check off
    a tile-decoder bug cannot hide behind the exact serial path."""
    names, blobs, caps = [], [], []
    for name, comp, raw in streams.valid_streams():
        if name == "fixed_sym286_is_eob":
            continue
        for c in (len(raw), len(raw) + 100):
            names.append("%s@%d" % (name, c))
            blobs.append(comp)
            caps.append(c)
    # 256: span decoder (experimental); 0x400: without the interval kernel; 0x1000: without the LZ-window
    # kernel (the tile decoders take the general streams, as before round 4); round 5: 0x10000 without the
    # landing decoder, 0x80000 the landing decoder with the general writing pass only, 0x100000 one stream
    for flags in (8, 4 | 8, 2, 16, 16 | 8, 128, 128 | 8, 256, 256 | 8, 256 | 4 | 8, 0x400, 0x400 | 8, 0x1000, 0x1000 | 8,
                  0x10000, 0x10000 | 8, 0x80000, 0x80000 | 8, 0x100000):
        harness.assert_inflate_parity(names, blobs, caps, flags=flags)


def test_landing_decoder_alone(harness):
    """inflate_seg3_kernel on its own (FDH_FLAG_LANDING_ONLY: what it leaves stays PENDING), with its lean
    and with the general writing pass: every stream it reports is right -- status, length, bytes, Adler-32
    against the oracle -- and it takes every ultra-fast stream up to 70 000 bytes (but the empty buffer's: shorter
    than the fixed prefix + 44 bits, left to the interval kernel) of the bench's three kinds of buffers (noisy
    rows, every other row zero, all zero), short ones and long ones, in exact and loose slots, at every
    alignment of input and slot (the harness packs back to back with odd guard slots in between)."""
    from fdeflate_amd import synth
    names, blobs, caps = [], [], []
    for sid, ln in ((0, 65536), (1, 65536), (7, 65536), (15, 65536), (3, 20000), (4, 300), (5, 0), (9, 200000), (23, 131072),
                    (31, 70000), (2, 4096), (6, 9), (8, 1023), (10, 1024), (11, 1025)):
        raw = synth.gen_stream_np(sid, ln).tobytes()
        comp = ob.compress_ultra_fast(raw)
        for c in (ln, ln + 17):
            names.append("uf%d_%d@%d" % (sid, ln, c))
            blobs.append(comp)
            caps.append(c)
    rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
    for flags in (0x20000, 0x20000 | 0x80000):
        st, ln_, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags)
        assert guards_ok
        passed_on = []
        for i, name in enumerate(names):
            if st[i] == 0xFFFFFFFF:
                passed_on.append(name)
                continue
            assert int(st[i]) == rs[i] == 0, (name, int(st[i]), rs[i], flags)
            assert int(ln_[i]) == rl[i] and outs[i][:rl[i]].tobytes() == ro[i] and int(ad[i]) == ra[i], (name, flags)
        # what it may pass on: streams shorter than the fixed prefix + 44 bits -- the empty buffer -- and the 200 000-byte
        # one, whose lanes' shares outgrow the check-point slots; nothing else of this list (a regression that sends the
        # bench's 64 KiB streams to the interval kernel would only show as speed)
        assert all(n_.startswith(("uf5_0@", "uf9_200000@")) for n_ in passed_on), (passed_on, flags)


def test_landing_decoder_flat_stretches(harness):
    """Run chains of every shape through inflate_seg3_kernel alone (FDH_FLAG_LANDING_ONLY), lean and general writing
    pass: zero runs from a few bytes to the whole buffer (the counting pass merges up to 64 tokens of 258 bytes into a
    chain and takes five of them per step; the lean writer keeps such chains out of its image and stores their zeros
    straight to the slot), at the start, in the middle and at the end of a buffer, back to back with a literal in
    between, across the lanes' segment borders -- and runs of a byte that is not zero, which the encoder writes as
    literals (src/compress/ultrafast.rs:94-167) so that they are no runs at all.  Everything the kernel reports must be
    the oracle's answer, and it must take every one of these streams (but the ones with thousands of equal literals in
    a row: the guessed chains of the lanes inside such a periodic stretch need not fall in step, and a stream whose
    lanes do not land after four rounds is the interval kernel's)."""
    r = np.random.default_rng(606)

    def noisy(n):
        x = r.integers(0, 256, n, dtype=np.uint8)
        x[r.random(n) < 0.3] = 0
        return x

    raws, periodic = [], set()
    for total in (65536, 70000):
        for run in (5, 8, 257, 258, 259, 260, 516, 517, 1024, 1290, 1291, 258 * 5 + 1, 258 * 6 + 1, 258 * 64 + 1, 258 * 64 + 2,
                    258 * 65 + 7, 258 * 128 + 1, 40000):
            if run + 200 > total:
                continue
            for at in (0, 1, 8, 4097, total - run - 100, total - run):
                x = noisy(total)
                x[at:at + run] = 0
                raws.append(x.tobytes())
        x = noisy(total)              # every other KiB flat (the bench's "half-zero" kind), and with a single literal between
        for k in range(0, total - 2048, 2048):
            x[k + 1024:k + 2048] = 0
        raws.append(x.tobytes())
        y = np.zeros(total, dtype=np.uint8)
        y[::1033] = 7
        raws.append(y.tobytes())
        raws.append(np.zeros(total, dtype=np.uint8).tobytes())
        z = noisy(total)
        z[1000:9000] = 5              # no run tokens: the encoder's runs are runs of zeros
        raws.append(z.tobytes())
        periodic.add(len(raws) - 1)
    for n in (2064, 2065, 4128, 16512, 16513, 16514, 33025, 66049, 300000, 1 << 20):
        raws.append(bytes(n))
        if n > 100000:  # (flat over several lanes' shares: the same token again and again is periodic too)
            periodic.add(len(raws) - 1)
    y = np.zeros(300000, dtype=np.uint8)
    y[::4099] = 1
    raws.append(y.tobytes())
    periodic.add(len(raws) - 1)
    names, blobs, caps, kinds = [], [], [], []
    for k, raw in enumerate(raws):
        comp = ob.compress_ultra_fast(raw)
        assert zlib.decompress(comp) == raw
        for c in (len(raw), len(raw) + 16):
            names.append("flat%d@%d" % (k, c))
            blobs.append(comp)
            caps.append(c)
            kinds.append(k in periodic)
    rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
    for flags in (0x20000, 0x20000 | 0x80000, 0):
        st, ln_, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags)
        assert guards_ok
        for i, name in enumerate(names):
            if int(st[i]) == 0xFFFFFFFF:
                assert flags != 0 and kinds[i], (name, "passed on", flags)
                continue
            assert int(st[i]) == rs[i] == 0, (name, int(st[i]), rs[i], flags)
            assert int(ln_[i]) == rl[i] and outs[i][:rl[i]].tobytes() == ro[i] and int(ad[i]) == ra[i], (name, flags)


def test_chain_behind_the_landing_decoder_long_short_and_chosen(harness):
    """What the landing decoder leaves over goes through five kernels (interval, segment, tile decoders, two exact kernels)
    or -- while recent calls left next to nothing -- through the exact kernel alone (fdh_launch_inflate, TailHint: the
    kernels report the count to mapped host memory, no synchronisation).  A batch large enough for the ordered path
    (16 384 streams and more), bench buffers, forty of them replaced by streams the landing decoder passes on (thousands
    of equal literals in a row): forced long, forced short and chosen, every stream must come back as it went in (the
    oracle checks a sample and the hard ones); and the choice must follow the reports -- short after calls that left
    nothing, long again after one that left many."""
    import ctypes as C
    import torch
    import bench
    import fdeflate_amd as fd
    from fdeflate_amd import synth, _lib, api
    lib = _lib.lib()
    r = np.random.default_rng(707)
    n, L, dev = 16400, 65536, torch.device("cuda", 0)
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    clean = synth.gen_batch_torch(50000, n, L, device=dev)
    mixed = clean.clone()
    hard_at = sorted(int(x) for x in r.choice(n, 40, replace=False))
    for k in hard_at:
        z = r.integers(0, 256, L, dtype=np.uint8)
        z[r.random(L) < 0.3] = 0
        a = int(r.integers(0, 40000))
        z[a:a + int(r.integers(6000, 20000))] = int(r.integers(1, 256))
        mixed[k] = torch.from_numpy(z).to(dev)

    def state():
        a = (C.c_uint * 4)()
        assert lib.fdh_debug_tail_state(a) == 0
        return list(a)

    def run(raw, flags, sample):
        comp, c_off, clen = bench.encode_ultrafast(raw, r_off, dev)
        out = torch.full((n * L,), 0xA5, dtype=torch.uint8, device=dev)
        ol, st, ad = fd.inflate_batch(comp, c_off, out, r_off, flags=flags)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0 and int((ol != L).sum()) == 0, (flags, int((st != 0).sum()))
        assert torch.equal(out.view(n, L), raw), flags
        ch, coh = comp.cpu().numpy(), c_off.cpu().numpy()
        adh = ad.cpu().numpy().view(np.uint32)
        for i in sample:
            blob = ch[int(coh[i]):int(coh[i]) + int(clen[i])].tobytes()
            s_, o_, a_ = ob.decompress_bounded(blob, L)
            assert s_ == 0 and o_ == raw[i].cpu().numpy().tobytes() and a_ == int(adh[i]), (flags, i)

    sample = list(range(0, n, 997)) + hard_at
    run(mixed, api.FLAG_TAIL_LONG, sample)
    run(mixed, api.FLAG_TAIL_SHORT, sample)
    for _ in range(3):          # nothing left over, three times (each call synchronised): the short chain is chosen
        run(clean, 0, sample[:4])
    assert state()[3] == 1, state()
    run(mixed, 0, hard_at)      # ... and it takes the forty streams as well (slowly); its report switches back
    assert state()[0] >= 20, state()
    run(clean, 0, sample[:4])
    assert state()[3] == 0, state()
    for _ in range(3):
        run(clean, 0, sample[:4])
    assert state()[3] == 1, state()


def _lz_cases():
    """General zlib streams for the LZ-window kernel (inflate_lz.h): every zlib level and strategy on the
    bench's buffers (noisy, half zero, all zero), short and long inputs, several blocks, text, matches that
    repeat themselves, distances up to 32 KiB, megabyte streams of very short codes."""
    import random
    import zlib
    from fdeflate_amd import synth
    rnd = random.Random(5)
    cases = [(n, c, r) for n, c, r in streams.valid_streams() if n != "fixed_sym286_is_eob"]
    for lvl in (1, 4, 6, 9):
        for sid, ln in ((0, 65536), (7, 65536), (15, 65536), (3, 20000), (4, 300), (9, 200000)):
            raw = synth.gen_stream_np(sid, ln).tobytes()
            cases.append(("zlib%d_s%d_%d" % (lvl, sid, ln), zlib.compress(raw, lvl), raw))
    for strat, sname in ((zlib.Z_FIXED, "fixed"), (zlib.Z_RLE, "rle"), (zlib.Z_HUFFMAN_ONLY, "huff"), (zlib.Z_FILTERED, "filt")):
        raw = synth.gen_stream_np(11, 50000).tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strat)
        cases.append(("strat_" + sname, c.compress(raw) + c.flush(), raw))
    text = (b"the quick brown fox jumps over the lazy dog " * 400) + bytes(rnd.randrange(256) for _ in range(3000))
    cases.append(("text", zlib.compress(text * 5, 6), text * 5))
    raw = b"ab" * 5000 + b"xyz" * 3000 + b"q" * 70000
    cases.append(("overlap", zlib.compress(raw, 9), raw))
    raw = bytes(rnd.randrange(256) for _ in range(200)) + bytes(30000) + bytes(rnd.randrange(4) for _ in range(40000))
    cases.append(("far", zlib.compress(raw, 6), raw))
    raw = bytes(1 << 20)
    cases.append(("zeros1M", zlib.compress(raw, 6), raw))
    raw = bytes(rnd.randrange(3) for _ in range(1 << 20))
    cases.append(("rand3_1M", zlib.compress(raw, 6), raw))
    return cases


def test_lz_window_kernel_alone(harness):
    """FDH_FLAG_LZ_ONLY (0x2000): nothing behind the LZ-window kernel runs, so what it reports is its own.
    It only ever reports Ok, and everything it reports is bit-exact with the oracle (bytes, length,
    Adler-32); what it leaves (stored blocks, slots that are too small) stays PENDING.  It must take the
    Huffman-only streams: dynamic and fixed blocks of every level / strategy."""
    cases = _lz_cases()
    names = [c[0] for c in cases]
    blobs = [c[1] for c in cases]
    for slack in (0, 100, -1):
        caps = [max(len(c[2]) + slack, 0) for c in cases]
        st, ln, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=0x2000)
        assert guards_ok, "the LZ-window kernel wrote outside a slot"
        rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
        took = 0
        for i, name in enumerate(names):
            if st[i] >= 0xFFFFFFFD:  # PENDING / PENDING_SERIAL / PENDING_RESUME: left to the kernels that did not run
                continue
            assert st[i] == 0 and rs[i] == 0, (name, int(st[i]), rs[i])
            took += 1
            assert int(ln[i]) == rl[i] and outs[i][:rl[i]].tobytes() == ro[i] and int(ad[i]) == ra[i], name
        if slack >= 0:
            must = [n for n in names if n.startswith(("zlib", "strat_", "text", "overlap", "far", "zeros1M", "rand3"))]
            left = [names[i] for i in range(len(names)) if st[i] >= 0xFFFFFFFD and names[i] in must]
            assert not left, left
        # (slack -1: a slot that is too small is the exact kernels' business -- whatever is reported Ok here,
        #  e.g. an empty stream in an empty slot by the kernels in front, agreed with the oracle above)
    # the whole pipeline on the same streams, with and without this kernel
    caps = [len(c[2]) for c in cases]
    harness.assert_inflate_parity(names, blobs, caps)
    harness.assert_inflate_parity(names, blobs, caps, flags=0x1000)


def test_zlib6_batch_at_scale_against_the_oracle(harness):
    """SURVEY 8(d) C2 (ii) as a test: 16 384 zlib level-6 streams of the bench's buffers (two dynamic
    blocks each, real distances up to 32 KiB, codes up to 14 bits) in one batch; status, length, Adler-32
    and every byte of every stream against the oracle (and the raw buffers), exact slots."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    n, L = 16384, 65536
    raw = synth.gen_batch_torch(0, n, L, device="cuda")
    h = raw.cpu().numpy()
    with ThreadPoolExecutor(16) as pool:
        blobs = list(pool.map(lambda i: zlib.compress(h[i].tobytes(), 6), range(n), chunksize=64))
    clen = np.array([len(b) for b in blobs], dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum((clen + 15) & ~15)
    buf = np.zeros(int(off[-1]), dtype=np.uint8)
    for i, b in enumerate(blobs):
        buf[off[i]:off[i] + len(b)] = np.frombuffer(b, dtype=np.uint8)
    comp, c_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()
    r_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    for flags in (0, 0x2000):  # the whole pipeline; the LZ-window kernel alone must finish all of them
        out = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
        out_len, status, adler = fd.inflate_batch(comp, c_off, out, r_off, flags=flags)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0, flags
        assert bool((out_len == L).all())
        assert torch.equal(out, raw.view(-1))
        ad = adler.cpu().numpy().view(np.uint32)
        ho = out.cpu().numpy()
        for i in range(n):
            st, dec, a = ob.decompress_bounded(blobs[i], L)
            assert st == 0 and a == int(ad[i]), i
            if i % 64 == 0:
                assert dec == ho[i * L:(i + 1) * L].tobytes(), i


def test_segment_kernel_long_canonical_streams(harness):
    """Long ultra-fast streams take the segment-parallel kernel (>= ~8 KiB compressed).  Every
    content class, odd lengths, exact / loose / short slots, plus corrupted and truncated copies
    that must fall through to the exact kernels with the reference's status."""
    from fdeflate_amd import synth
    r = np.random.default_rng(77)
    raws = []
    for i in (0, 1, 7, 15, 16, 23, 40):
        raws.append(synth.gen_stream_np(i, 65536).tobytes())
    raws.append(synth.gen_stream_np(2, 65536, "M").tobytes())
    raws.append(synth.gen_stream_np(3, 65536, "L").tobytes())
    raws.append(synth.gen_stream_np(4, 65536, "U").tobytes())
    raws.append(r.integers(0, 256, 30011, dtype=np.uint8).tobytes())
    raws.append((r.integers(0, 256, 70001, dtype=np.uint8) % 3).astype(np.uint8).tobytes())
    for n in (20000, 65536, 131072 + 5):
        x = r.integers(0, 256, n, dtype=np.uint8)
        x[r.random(n) < 0.6] = 0
        raws.append(x.tobytes())
        y = r.integers(1, 256, n, dtype=np.uint8)   # no zeros at all: literals only
        raws.append(y.tobytes())
        z = x.copy()
        z[n // 3: n // 3 + 5000] = 0                # one long run in the middle
        raws.append(z.tobytes())
    names, blobs, caps = [], [], []
    for k, raw in enumerate(raws):
        comp = ob.compress_ultra_fast(raw)
        for c in (len(raw), len(raw) + 33, len(raw) - 1, len(raw) // 2):
            names.append("seg%d@%d" % (k, c))
            blobs.append(comp)
            caps.append(c)
        bad = bytearray(comp)
        bad[len(bad) // 2] ^= 0x10
        names.append("seg%d_flip" % k)
        blobs.append(bytes(bad))
        caps.append(len(raw) + 100)
        bad = bytearray(comp)
        bad[-2] ^= 0x01
        names.append("seg%d_adler" % k)
        blobs.append(bytes(bad))
        caps.append(len(raw))
        names.append("seg%d_trunc" % k)
        blobs.append(comp[:len(comp) * 2 // 3])
        caps.append(len(raw))
    harness.assert_inflate_parity(names, blobs, caps)
    harness.assert_inflate_parity(names, blobs, caps, flags=0x400)        # without the interval kernel
    harness.assert_inflate_parity(names, blobs, caps, flags=128)          # without both segment-parallel kernels
    harness.assert_inflate_parity(names, blobs, caps, flags=1)            # ignore_adler32
    harness.assert_inflate_parity(names, blobs, caps, flags=1 | 0x400)


def test_segment_kernel_alone_short_and_unaligned(harness):
    """The segment-parallel kernel on its own (FDH_FLAG_FIRST_ONLY): canonical streams of every
    small size, at odd slot alignments.  It may leave a stream PENDING, but whatever it reports as
    Ok must be the reference's answer -- and it must take the plain cases."""
    from fdeflate_amd import synth
    r = np.random.default_rng(5)
    raws = [b"", b"a", b"\x00", b"\x00" * 5, b"\x00" * 258, b"\x00" * 259, b"\x00" * 100000, b"ab" * 700]
    for n in list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 1000, 1023, 1024, 1025,
                                   2047, 2048, 4095, 4096, 4097, 9000, 20000]:
        raws.append(r.integers(0, 256, n, dtype=np.uint8).tobytes())
        x = r.integers(0, 256, n, dtype=np.uint8)
        x[r.random(n) < 0.7] = 0
        raws.append(x.tobytes())
    raws.append(synth.gen_stream_np(3, 4096).tobytes())
    names, blobs, caps = [], [], []
    for k, raw in enumerate(raws):
        comp = ob.compress_ultra_fast(raw)
        for c in (len(raw), len(raw) + 7, max(len(raw) - 1, 0)):
            names.append("s%d@%d" % (k, c))
            blobs.append(comp)
            caps.append(c)
        names.append("s%d_trunc" % k)
        blobs.append(comp[:-3])
        caps.append(len(raw))
    rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
    plain = sum(1 for i in range(len(names)) if rs[i] == 0)
    # 0x800: the interval kernel alone; 0x400 | 64: the segment kernel alone; 64: both
    for flags in (0x800, 0x400 | 64, 64):
        st, ln, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags)
        assert guards_ok, "a segment-parallel kernel wrote outside a slot (flags %#x)" % flags
        taken = 0
        for i, name in enumerate(names):
            assert int(st[i]) in (0, 15, 0xFFFFFFFF), (name, int(st[i]))
            if int(st[i]) == 15:  # (a wrong trailer behind a stream that decoded to its end: classified on the spot)
                assert rs[i] == 15, (name, "reported WrongChecksum, reference says", ob.STATUS_NAMES[rs[i]])
            if int(st[i]) == 0:
                taken += 1
                assert rs[i] == 0, (name, "reported Ok, reference says", ob.STATUS_NAMES[rs[i]])
                assert int(ln[i]) == rl[i] and outs[i][:rl[i]].tobytes() == ro[i] and int(ad[i]) == ra[i], name
        assert taken >= 0.9 * plain, (flags, taken, plain)


def test_segment_kernel_random_stress(harness):
    """Many random canonical streams (sizes 0..200 KiB, zero density 0..100 %, long runs, exact /
    loose / short slots, corrupted and truncated copies) against the oracle, through the full
    pipeline and with the segment kernel's result taken alone."""
    r = np.random.default_rng(2024)
    names, blobs, caps = [], [], []
    for k in range(400):
        n = int(r.choice([r.integers(0, 300), r.integers(300, 5000), r.integers(5000, 70000), r.integers(70000, 200000)]))
        dens = float(r.choice([0.0, 0.1, 0.5, 0.9, 0.99, 1.0]))
        x = r.integers(0, 256, n, dtype=np.uint8)
        if r.random() < 0.5:
            x = (x % int(r.choice([2, 4, 17, 64]))).astype(np.uint8)
        x[r.random(n) < dens] = 0
        if n > 600 and r.random() < 0.5:
            a = int(r.integers(0, n - 500))
            x[a:a + int(r.integers(1, 500))] = int(r.integers(0, 256))  # a run of a non-zero byte is NOT a run token
        raw = x.tobytes()
        comp = ob.compress_ultra_fast(raw)
        mode = k % 5
        if mode == 0:
            cap = n
        elif mode == 1:
            cap = n + int(r.integers(1, 100))
        elif mode == 2:
            cap = max(0, n - int(r.integers(1, 50)))
        elif mode == 3:
            cap = n
            b = bytearray(comp)
            b[int(r.integers(2, len(b)))] ^= 1 << int(r.integers(0, 8))
            comp = bytes(b)
        else:
            cap = n
            comp = comp[:int(r.integers(1, len(comp)))]
        names.append("r%d_m%d_n%d" % (k, mode, n))
        blobs.append(comp)
        caps.append(cap)
    harness.assert_inflate_parity(names, blobs, caps)
    harness.assert_inflate_parity(names, blobs, caps, flags=0x400)
    rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
    for flags in (0x800, 0x400 | 64):   # the interval kernel alone, the segment kernel alone
        st, ln, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags)
        assert guards_ok
        for i, name in enumerate(names):
            # (Ok, left for the kernels behind, or -- round 4 -- WrongChecksum: a stream decoded to its end whose
            #  trailer is there and differs is classified on the spot)
            assert int(st[i]) in (0, 15, 0xFFFFFFFF), (name, int(st[i]))
            if int(st[i]) == 0:
                assert rs[i] == 0 and int(ln[i]) == rl[i] and outs[i][:rl[i]].tobytes() == ro[i] and int(ad[i]) == ra[i], name
            if int(st[i]) == 15:
                assert rs[i] == 15, (name, rs[i])


def test_valid_streams_ignore_adler(harness):
    names, blobs, caps = [], [], []
    for name, comp, raw in streams.valid_streams():
        bad = bytearray(comp)
        bad[-1] ^= 0xFF
        names.append(name)
        blobs.append(bytes(bad))
        caps.append(len(raw) + 3)
    harness.assert_inflate_parity(names, blobs, caps, flags=1)
    harness.assert_inflate_parity(names, blobs, caps, flags=0)  # -> WrongChecksum everywhere


def test_reference_vectors_corpus_and_zz(harness, golden_manifest):
    items = streams.corpus_streams()
    names = [n for n, _ in items]
    blobs = [b for _, b in items]
    caps = [1 << 16] * len(items)
    harness.assert_inflate_parity(names, blobs, caps)
    harness.assert_inflate_parity(names, blobs, caps, flags=1)
    # the literal expectations of the reference tests (src/decompress.rs:1344-1384)
    st, ln, ad, outs, ok = harness.gpu_inflate(blobs, caps, flags=1)
    by = dict(zip(names, zip(st, ln, ad)))
    assert tuple(int(x) for x in by["zz_example1"]) == (0, 281, 751299)
    assert int(by["zz_example2"][0]) == 9 and int(by["zz_example3"][0]) == 9
    for name, exp in golden_manifest["corpus"].items():
        s, l, a = by["corpus_" + name[:8]]
        assert (int(s), int(l), int(a)) == (0, exp["length"], exp["adler32"])


def test_error_streams(harness):
    items = streams.error_streams()
    names = [n for n, _, _ in items]
    blobs = [b for _, b, _ in items]
    for cap in (1 << 16, 4, 0):
        harness.assert_inflate_parity(names, blobs, [cap] * len(items))
    harness.assert_inflate_parity(names, blobs, [1 << 16] * len(items), flags=16)  # via the lane kernel
    st, _, _, _, _ = harness.gpu_inflate(blobs, [1 << 16] * len(items))
    for (name, _, expect), s in zip(items, st):
        assert ob.STATUS_NAMES[int(s)] == expect, (name, ob.STATUS_NAMES[int(s)], expect)


def test_mutation_fuzz_parity(harness):
    items = streams.mutation_streams(n_per_seed=60, seeds=(11, 12, 13, 14))
    names = [n for n, _ in items]
    blobs = [b for _, b in items]
    for cap in (1 << 16, 1000):
        harness.assert_inflate_parity(names, blobs, [cap] * len(items))
        harness.assert_inflate_parity(names, blobs, [cap] * len(items), flags=16)


def test_truncation_sweep(harness):
    """every prefix of a few streams: InsufficientInput/OutputTooLarge/errors exactly as the
    reference's one-shot wrapper classifies them"""
    bases = [zlib.compress(bytes(range(256)) * 3, 6), ob.compress_ultra_fast(b"Hello world! " * 9),
             ob.compress_stored(b"stored block payload " * 4)]
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    bases.append(c.compress(b"fixed fixed fixed fixed") + c.flush())
    names, blobs = [], []
    for bi, base in enumerate(bases):
        for cut in range(len(base) + 1):
            names.append("b%d_cut%d" % (bi, cut))
            blobs.append(base[:cut])
    for cap in (1 << 12, 100, 24):
        harness.assert_inflate_parity(names, blobs, [cap] * len(blobs))
        harness.assert_inflate_parity(names, blobs, [cap] * len(blobs), flags=16)


def _damaged_long_cases():
    """Long streams cut short, bit-flipped and with damaged trailers: the cases whose classification the exact
    serial decoder owns.  Several tiles / blocks lie in front of the damage, so the decoder re-derives the
    result from a check point in the middle of the stream."""
    import random
    from fdeflate_amd import synth
    rnd = random.Random(77)
    noisy = synth.gen_stream_np(0, 65536).tobytes()
    half = synth.gen_stream_np(15, 40000).tobytes()
    text = (b"it was the best of times, it was the worst of times, " * 300) + bytes(rnd.randrange(256) for _ in range(5000))
    bases = [("zlib6", zlib.compress(noisy, 6)), ("zlib1", zlib.compress(half, 1)), ("zlib9text", zlib.compress(text, 9))]
    for strat, sname in ((zlib.Z_FIXED, "fixed"), (zlib.Z_HUFFMAN_ONLY, "huff"), (zlib.Z_RLE, "rle")):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strat)
        bases.append((sname, c.compress(noisy[:30000]) + c.flush()))
    bases.append(("uf", ob.compress_ultra_fast(noisy)))
    bases.append(("uf_half", ob.compress_ultra_fast(half)))
    bases.append(("stored", ob.compress_stored(noisy + noisy[:5000])))
    c = zlib.compressobj(6)
    multi = b"".join(c.compress(noisy[k:k + 9000]) + c.flush(zlib.Z_FULL_FLUSH) for k in range(0, 63000, 9000)) + c.flush()
    bases.append(("flushes", multi))
    names, blobs = [], []
    for bname, base in bases:
        cuts = sorted(set([rnd.randrange(2, len(base)) for _ in range(24)] + list(range(len(base) - 12, len(base)))))
        for cut in cuts:
            names.append("%s_cut%d" % (bname, cut))
            blobs.append(base[:cut])
        for k in range(16):
            b = bytearray(base)
            at = rnd.randrange(len(b) // 2, len(b)) if k % 2 else len(b) - 1 - rnd.randrange(6)
            b[at] ^= 1 << rnd.randrange(8)
            names.append("%s_flip%d" % (bname, at))
            blobs.append(bytes(b))
    return names, blobs


def test_damaged_long_streams_rederived_from_a_check_point(harness):
    """inflate_general_kernel re-derives a doubtful result with the exact serial decoder from its last check
    point (a block header or the start of a tile) instead of the stream's first byte: same status, length
    and Adler-32 as the oracle for cuts, bit flips and damaged trailers far into long streams -- with the
    check points (default), without them (FDH_FLAG_NO_CHECKPOINTS, 0x4000: the serial pass over the whole
    stream of rounds 1-3), and with the LZ-window kernel out of the way (0x1000)."""
    names, blobs = _damaged_long_cases()
    import random
    rnd = random.Random(3)
    for caps in ([1 << 17] * len(blobs), [rnd.choice((65536, 40000, 30000, 12345, 1000)) for _ in blobs]):
        # what `read` had produced when the input ran out (the streaming object relies on that length)
        partial = {}
        for i, blob in enumerate(blobs):
            d = ob.Decompressor()
            out = np.zeros(caps[i], dtype=np.uint8)
            st, c, p = d.read(blob, out, 0)
            if st == 0 and not d.is_done() and p < caps[i]:
                partial[i] = out[:p].tobytes()
        assert len(partial) > 100
        for flags in (0, 0x4000, 0x1000, 0x1000 | 0x4000):
            harness.assert_inflate_parity(names, blobs, caps, flags=flags)
            st, ln, ad, outs, ok = harness.gpu_inflate(blobs, caps, flags)
            for i, data in partial.items():
                assert int(st[i]) == 2, (names[i], int(st[i]), flags)
                assert int(ln[i]) == len(data) and outs[i][:len(data)].tobytes() == data, (names[i], int(ln[i]), len(data), flags)


def test_dense_cuts_of_pair_heavy_streams(harness):
    """Every cut in two windows of streams whose literals nearly all pair up in the reference's table (two
    literals per table step, src/huffman.rs:110-130): where `read` stops when the input runs out depends on
    which literals were paired (src/decompress.rs:852), i.e. on the parity of the whole chain of steps in front
    of the cut.  The tile decoders follow that chain through every tile (STEP_START / STEP_SECOND at a check
    point, inflate_stream.h); one slip and the length reported for InsufficientInput is off by one."""
    from fdeflate_amd import synth
    noisy = synth.gen_stream_np(0, 65536).tobytes()
    small = bytes((b % 7) for b in noisy[:40000])          # seven symbols: two- and three-bit codes, no matches wanted
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    bases = [ob.compress_ultra_fast(noisy), c.compress(small) + c.flush(), zlib.compress(small, 6)]
    names, blobs, exp = [], [], []
    for bi, base in enumerate(bases):
        for lo in (len(base) // 9, (len(base) * 2) // 3):
            for cut in range(lo, lo + 300):
                d = ob.Decompressor()
                out = np.zeros(1 << 17, dtype=np.uint8)
                st, cons, p = d.read(base[:cut], out, 0)
                assert st == 0 and not d.is_done()
                names.append("b%d_cut%d" % (bi, cut))
                blobs.append(base[:cut])
                exp.append(out[:p].tobytes())
    caps = [1 << 17] * len(blobs)
    for flags in (0, 0x4000, 0x1000):
        st, ln, ad, outs, ok = harness.gpu_inflate(blobs, caps, flags)
        assert ok
        bad = [(names[i], int(st[i]), int(ln[i]), len(exp[i])) for i in range(len(blobs))
               if int(st[i]) != 2 or int(ln[i]) != len(exp[i]) or outs[i][:len(exp[i])].tobytes() != exp[i]]
        assert not bad, (flags, len(bad), bad[:8])


def test_ultrafast_encode_bit_exact(harness):
    import fdeflate_amd as fd
    r = np.random.default_rng(99)
    raws = [b"", b"Hello world!", bytes(1), bytes(7), bytes(8), bytes(9), bytes(2048), bytes([5]) * 2048,
            bytes([128]) * 2048, bytes([254]) * 2048, bytes(65536), b"\x01" + bytes(300) + b"\x02",
            bytes(258 * 3 + 6), bytes(8) + b"\x01" + bytes(7), b"\x00\x00\x05" + bytes(5) + bytes(16) + b"\x09"]
    for n in (1, 2, 3, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1000, 4096, 65536, 70001):
        x = r.integers(0, 256, n, dtype=np.uint8)
        raws.append(x.tobytes())
        y = x.copy()
        y[r.random(n) < 0.7] = 0
        raws.append(y.tobytes())
        z = x.copy()
        z[r.random(n) < 0.97] = 0
        raws.append(z.tobytes())
    from fdeflate_amd import synth
    for i in (0, 1, 7, 15, 16, 23):
        raws.append(synth.gen_stream_np(i, 65536).tobytes())
    raws.append(bytes(3_000_000) + b"\x07" + bytes(100))  # a run too long for the LDS bit ring
    # around and beyond 256 tiles (128 KiB), where the 32-bit Adler partial sums are folded; 0xFF is their worst case
    for n in (131071, 131072, 131073, 131072 * 3 + 5, (1 << 20) + 3):
        raws.append(bytes([255]) * n)
        x = r.integers(0, 256, n, dtype=np.uint8)
        x[r.random(n) < 0.3] = 0
        raws.append(x.tobytes())
    res, ok = harness.gpu_deflate(raws)
    assert ok
    for i, raw in enumerate(raws):
        exp = ob.compress_ultra_fast(raw)
        assert res[i] == exp, (i, len(raw), len(res[i]), len(exp))
    # single-buffer convenience (host memory) mirrors compress_to_vec_ultra_fast
    assert fd.compress_to_vec_ultra_fast(b"Hello world!") == ob.compress_ultra_fast(b"Hello world!")


def test_stored_encode_bit_exact(harness):
    """Level 0 (compress_to_vec_with_level(.., 0)): bit-exact with the oracle's restatement for the
    block-boundary sizes, the batch and the host entry points, and it decodes back."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(11)
    sizes = [0, 1, 7, 8, 9, 4096, 65534, 65535, 65536, 65535 * 2 - 1, 65535 * 2, 65535 * 2 + 1, 200003]
    raws = [r.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    want = [ob.compress_stored(x) for x in raws]
    assert want[0] == bytes.fromhex("7801030000000001")  # the reference's empty-input KAT (level 0 = level 1 here)
    for x, w in zip(raws, want):
        assert fd.stored_size(len(x)) == len(w)
    for x, w in zip(raws[:6], want[:6]):
        assert fd.compress_to_vec_stored(x) == w
    # batch, unaligned packing, guard bytes between the slots
    buf, in_off = streams.pack_exact(raws)
    caps = [fd.stored_size(len(x)) + 3 for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
    ln = fd.deflate_stored_batch(torch.as_tensor(buf).cuda(), torch.as_tensor(in_off.astype(np.int64)).cuda(), d_out,
                                 torch.as_tensor(out_off).cuda())
    torch.cuda.synchronize()
    h = d_out.cpu().numpy()
    for i, w in enumerate(want):
        o0 = int(out_off[i])
        assert int(ln[i]) == len(w), (sizes[i], int(ln[i]), len(w))
        assert h[o0:o0 + len(w)].tobytes() == w, sizes[i]
        assert np.all(h[o0 + len(w):int(out_off[i + 1])] == 0x5A), sizes[i]
    # too small a slot is refused, nothing else is touched
    small = torch.full((10,), 0x5A, dtype=torch.uint8, device="cuda")
    ln = fd.deflate_stored_batch(torch.as_tensor(np.frombuffer(raws[3], dtype=np.uint8).copy()).cuda(),
                                 torch.tensor([0, 8], dtype=torch.int64, device="cuda"), small,
                                 torch.tensor([0, 10], dtype=torch.int64, device="cuda"))
    assert int(ln[0]) == -1 or int(ln[0]) == 0xFFFFFFFF
    # and the decoder takes them (stored blocks through the general kernels)
    names = ["stored%d" % n for n in sizes]
    harness.assert_inflate_parity(names, want, [len(x) for x in raws])


def test_host_api_mirror(harness):
    import fdeflate_amd as fd
    data = b"Hello world! " * 100
    assert fd.decompress_to_vec(zlib.compress(data)) == data
    assert fd.decompress_to_vec(fd.compress_to_vec_ultra_fast(data)) == data
    assert fd.decompress_to_vec_bounded(zlib.compress(data), len(data)) == data
    with pytest.raises(fd.OutputTooLarge) as ei:
        fd.decompress_to_vec_bounded(zlib.compress(data), 10)
    assert ei.value.partial_output == data[:10]
    with pytest.raises(fd.DecompressionError) as ei:
        fd.decompress_to_vec(zlib.compress(data)[:-3])
    assert ei.value.kind == "InsufficientInput"
    bad = bytearray(zlib.compress(data))
    bad[-1] ^= 1
    with pytest.raises(fd.DecompressionError) as ei:
        fd.decompress_to_vec(bytes(bad))
    assert ei.value.kind == "WrongChecksum"
    big = bytes(1 << 20)  # forces the slot-doubling loop of decompress_to_vec
    assert fd.decompress_to_vec(zlib.compress(big, 9)) == big


def test_c1_single_4k_stream_plumbing(harness):
    """BASELINE config 1: one 4 KiB stream.  The reference side is the oracle's streaming
    Decompressor (whole input and byte-at-a-time), the product side the batch-of-one GPU path."""
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    raw = synth.gen_stream_np(3, 4096, png_rows=False).tobytes()
    comp = ob.compress_ultra_fast(raw)
    assert ob.decompress_by_chunks(comp, 0) == (0, raw)
    assert ob.decompress_by_chunks(comp, 1) == (0, raw)
    assert fd.compress_to_vec_ultra_fast(raw) == comp
    assert fd.decompress_to_vec(comp) == raw


def test_mixed_batch_at_scale(harness):
    """BASELINE config 5 in miniature: a few thousand streams of every kind in ONE batch -- the
    corpus, stored / fixed / dynamic streams of every zlib strategy, ultra-fast streams, error and
    mutated streams -- interleaved, with exact / loose / short slots, so that every kernel of the
    pipeline and its PENDING hand-over (lists, counters) work side by side.  Bit-exact vs the oracle."""
    pool = []
    for name, comp, raw in streams.valid_streams():
        for c in (len(raw), len(raw) + 9, max(len(raw) - 1, 0)):
            pool.append((name + "@%d" % c, comp, c))
    for name, comp in streams.corpus_streams():
        pool.append((name, comp, 1 << 16))
    for item in streams.error_streams():
        pool.append(("err_" + item[0], item[1], 4096))
    for name, comp in streams.mutation_streams(n_per_seed=10, seeds=(7,)):
        pool.append(("mut_" + name, comp, 70000))
    r = np.random.default_rng(99)
    order = r.permutation(len(pool) * 4) % len(pool)   # every stream four times, shuffled
    names = [pool[i][0] + "#%d" % k for k, i in enumerate(order)]
    blobs = [pool[i][1] for i in order]
    caps = [pool[i][2] for i in order]
    assert len(names) > 1500
    harness.assert_inflate_parity(names, blobs, caps)


def test_ragged_batch_handed_out_long_streams_first(harness):
    """20 000 ultra-fast streams of very different lengths in one batch (most short, every eighth
    long, some empty, a few non-canonical ones in between): with several streams per persistent
    wavefront the interval kernel hands them out long ones first (stream_order_kernel) and sends the
    non-canonical ones straight to the general kernels' list.  Encode on the GPU, decode, compare
    with the raw bytes; the checksum the decoder reports must be the trailer the encoder wrote."""
    import torch
    import zlib
    import fdeflate_amd as fd
    r = np.random.default_rng(2026)
    n = 20000
    lens = r.integers(0, 3000, n)
    lens[::8] = r.integers(20000, 60000, len(lens[::8]))
    lens[5::97] = 0
    total = int(lens.sum())
    raw_h = r.integers(0, 256, total, dtype=np.uint8)
    raw_h[r.random(total) < 0.6] = 0
    r_off_h = np.zeros(n + 1, dtype=np.int64)
    r_off_h[1:] = np.cumsum(lens)
    raw = torch.from_numpy(raw_h).cuda()
    r_off = torch.from_numpy(r_off_h).cuda()
    bounds = np.array([(fd.ultrafast_bound(int(x)) + 15) & ~15 for x in lens], dtype=np.int64)
    c_off_h = np.zeros(n + 1, dtype=np.int64)
    c_off_h[1:] = np.cumsum(bounds)
    c_off = torch.from_numpy(c_off_h).cuda()
    comp = torch.zeros(int(c_off_h[-1]), dtype=torch.uint8, device="cuda")
    clen = fd.deflate_ultrafast_batch(raw, r_off, comp, c_off)
    # every 501st stream is replaced by a zlib level-6 stream of the same bytes (fits the slot: the
    # ultra-fast bound is larger than anything zlib produces for these sizes)
    comp_h = comp.cpu().numpy()
    clen_h = clen.cpu().numpy().astype(np.int64)
    swapped = list(range(3, n, 501))
    for i in swapped:
        z = zlib.compress(raw_h[r_off_h[i]:r_off_h[i + 1]].tobytes(), 6)
        assert len(z) <= bounds[i]
        comp_h[c_off_h[i]:c_off_h[i] + bounds[i]] = 0
        comp_h[c_off_h[i]:c_off_h[i] + len(z)] = np.frombuffer(z, dtype=np.uint8)
        clen_h[i] = len(z)
    comp = torch.from_numpy(comp_h).cuda()
    # (and the other list built in one launch / in two: the library chooses by what recent calls reported)
    for flags in (0, fd.api.FLAG_NO_INTERVALS, fd.api.FLAG_ORDER_ONCE, fd.api.FLAG_ORDER_TWICE, fd.api.FLAG_ORDER_ONCE | fd.api.FLAG_TAIL_SHORT):
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out_len, status, adler = fd.inflate_batch(comp, c_off, out, r_off, flags=flags)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0, flags
        assert torch.equal(out_len.to(torch.int64), torch.from_numpy(lens).cuda()), flags
        assert torch.equal(out[:total], raw), flags
        assert bool((out[total:] == 0xA5).all()), flags
        ad = adler.cpu().numpy().view(np.uint32)
        for i in list(range(0, n, 997)) + swapped[:5]:
            t = comp_h[c_off_h[i] + clen_h[i] - 4:c_off_h[i] + clen_h[i]]
            assert int(ad[i]) == int.from_bytes(t.tobytes(), "big"), (flags, i)


def test_batch_roundtrip_at_scale(harness):
    """4096 x 64 KiB: encode on the GPU, decode on the GPU; every stream Ok, lengths exact,
    decoded == raw, and the Adler-32 the decoder reports equals the trailer the encoder wrote
    (a checksum of checksums; the oracle spot-checks a sample bit-exactly)."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    n, L = 4096, 65536
    raw = synth.gen_batch_torch(0, n, L)
    assert np.array_equal(raw[5].cpu().numpy(), synth.gen_stream_np(5, L))
    bound = (fd.ultrafast_bound(L) + 15) & ~15
    in_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    c_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * bound
    comp = torch.zeros(n * bound, dtype=torch.uint8, device="cuda")
    clen = fd.deflate_ultrafast_batch(raw.view(-1), in_off, comp, c_off)
    torch.cuda.synchronize()
    clen_h = clen.cpu().numpy()
    for i in (0, 7, 15, 100, 4095):
        exp = ob.compress_ultra_fast(raw[i].cpu().numpy().tobytes())
        got = comp[i * bound:i * bound + int(clen_h[i])].cpu().numpy().tobytes()
        assert got == exp, i
    # decode from the padded slots (trailing bytes after the trailer are ignored by the format)
    out = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    out_len, status, adler = fd.inflate_batch(comp, c_off, out, in_off)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert bool((out_len == L).all())
    assert torch.equal(out, raw.view(-1))
    # trailer = last 4 bytes of each stream, big-endian
    idx = (c_off[:-1] + clen.to(torch.int64))[:, None] + torch.arange(-4, 0, device="cuda")[None, :]
    tr = comp[idx].to(torch.int64)
    trailer = (tr[:, 0] << 24) | (tr[:, 1] << 16) | (tr[:, 2] << 8) | tr[:, 3]
    assert torch.equal(trailer, adler.to(torch.int64) & 0xFFFFFFFF)


def _roundtrip_at_scale(n, first, dev="cuda", sample=()):
    """encode n x 64 KiB on the GPU, decode on the GPU, property checks at full size: every
    stream Ok, lengths exact, decoded == raw, reported Adler-32 == the trailer the encoder wrote
    (a checksum of checksums); the oracle byte-compares a strided sample of the COMPRESSED and of
    the DECODED streams."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    L = 65536
    raw = synth.gen_batch_torch(first, n, L, device=dev)
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    bound = (fd.ultrafast_bound(L) + 15) & ~15
    # lengths first (bound-sized slots in chunks), then the packed 16-B aligned layout of the bench
    clen = torch.empty(n, dtype=torch.int32, device=dev)
    chunk = 8192
    tmp = torch.empty(chunk * bound, dtype=torch.uint8, device=dev)
    t_off = torch.arange(chunk + 1, dtype=torch.int64, device=dev) * bound
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        fd.deflate_ultrafast_batch(raw[c0:c1].reshape(-1), r_off[:c1 - c0 + 1], tmp, t_off[:c1 - c0 + 1], clen[c0:c1])
    del tmp
    clen64 = clen.to(torch.int64)
    c_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    c_off[1:] = torch.cumsum((clen64 + 15) & ~15, 0)
    comp = torch.zeros(int(c_off[-1]), dtype=torch.uint8, device=dev)
    clen2 = fd.deflate_ultrafast_batch(raw.view(-1), r_off, comp, c_off)
    assert torch.equal(clen2, clen)
    out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    out_len, status, adler = fd.inflate_batch(comp, c_off, out, r_off)
    torch.cuda.synchronize(dev)
    assert int(status.abs().sum()) == 0
    assert bool((out_len == L).all())
    assert torch.equal(out, raw.view(-1))
    idx = (c_off[:-1] + clen64)[:, None] + torch.arange(-4, 0, device=dev)[None, :]
    tr = comp[idx].to(torch.int64)
    trailer = (tr[:, 0] << 24) | (tr[:, 1] << 16) | (tr[:, 2] << 8) | tr[:, 3]
    assert torch.equal(trailer, adler.to(torch.int64) & 0xFFFFFFFF)
    c_off_h = c_off.cpu().numpy()
    clen_h = clen.cpu().numpy()
    for i in sample:
        r = raw[i].cpu().numpy().tobytes()
        assert r == synth.gen_stream_np(first + i, L).tobytes()
        got = comp[int(c_off_h[i]):int(c_off_h[i]) + int(clen_h[i])].cpu().numpy().tobytes()
        assert got == ob.compress_ultra_fast(r), i
        st, dec, ad = ob.decompress_bounded(got, L)
        assert st == 0 and dec == out[i * L:(i + 1) * L].cpu().numpy().tobytes(), i
        assert ad == (int(adler[i]) & 0xFFFFFFFF)


def test_c2_full_size_batch(harness):
    """BASELINE config 2 at full size: 65 536 x 64 KiB through fdh_inflate_batch."""
    _roundtrip_at_scale(65536, 0, sample=range(0, 65536, 4099))


def test_c4_one_shard_of_the_million_stream_batch(harness):
    """BASELINE config 4 shards 1 048 576 streams over 8 GPUs: 131 072 streams per GPU (~4 GiB in,
    8 GiB out).  One such shard (rank 3's seeds) on this GPU."""
    _roundtrip_at_scale(131072, 3 * 131072, sample=range(5, 131072, 16381))


def test_mixed_batch_on_every_visible_device(harness):
    """BASELINE config 5's workload placed on cuda:k for every visible device while cuda:0 stays
    the current device (the entry points make the tensors' device current for the call)."""
    import torch
    import fdeflate_amd as fd
    pool = []
    for name, comp, raw in streams.valid_streams():
        pool.append((comp, len(raw) + 3))
    for name, comp in streams.corpus_streams():
        pool.append((comp, 1 << 16))
    for item in streams.error_streams():
        pool.append((item[1], 4096))
    blobs = [p[0] for p in pool]
    caps = [p[1] for p in pool]
    rs, rl, ra, ro = harness.oracle_inflate(blobs, caps)
    buf, in_off = streams.pack_exact(blobs)
    out_off = np.zeros(len(blobs) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(np.asarray(caps, dtype=np.int64))
    torch.cuda.set_device(0)
    for k in range(torch.cuda.device_count()):
        dev = torch.device("cuda", k)
        d_in = torch.from_numpy(buf).to(dev)
        d_in_off = torch.from_numpy(in_off.astype(np.int64)).to(dev)
        d_out = torch.zeros(int(out_off[-1]), dtype=torch.uint8, device=dev)
        d_out_off = torch.from_numpy(out_off).to(dev)
        out_len, status, adler = fd.inflate_batch(d_in, d_in_off, d_out, d_out_off)
        torch.cuda.synchronize(dev)
        assert torch.cuda.current_device() == 0
        st = status.cpu().numpy().view(np.uint32)
        ln = out_len.cpu().numpy().view(np.uint32)
        h = d_out.cpu().numpy()
        for i in range(len(blobs)):
            assert int(st[i]) == rs[i], (k, i)
            if rs[i] in (0, 17):
                assert int(ln[i]) == rl[i] and h[out_off[i]:out_off[i] + rl[i]].tobytes() == ro[i], (k, i)
    if torch.cuda.device_count() > 1:
        a = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        b = torch.zeros(2, dtype=torch.int64, device="cuda:1")
        with pytest.raises(ValueError):
            fd.inflate_batch(a, b, a, b)


def test_general_encoder_level1_and_rle_bit_exact(harness):
    """compress_to_vec (level 1) and compress_to_vec_rle on the GPU (parser kernel + block-writer
    kernel) against the oracle's restatement: bit-exact, batch and host conveniences, guard bytes
    behind every slot; inputs include several-block streams and trees that must be shortened to 15 /
    7 bits.  The parser is run with 1, 8 and 64 streams per wavefront (FDH_GEN_LANES; the library
    picks by batch size otherwise)."""
    import torch
    import fdeflate_amd as fd
    raws = streams.encoder_inputs()
    r = np.random.default_rng(17)
    for k in range(70):   # more than one wavefront of streams, ragged sizes
        n = int(r.integers(0, 9000))
        raws.append(bytes(r.integers(0, int(r.integers(2, 256)), n, dtype=np.uint8)))
    assert fd.compress_to_vec(b"") == bytes.fromhex("7801030000000001")
    assert fd.compress_to_vec(b"Hello world!") == ob.compress_level1(b"Hello world!")
    assert fd.compress_to_vec_rle(bytes(3000)) == ob.compress_rle(bytes(3000))
    buf, in_off = streams.pack_exact(raws)
    caps = [fd.compress_bound(len(x)) + 5 for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_in = torch.from_numpy(buf).cuda()
    d_in_off = torch.from_numpy(in_off.astype(np.int64)).cuda()
    d_out_off = torch.from_numpy(out_off).cuda()
    expect = {fd.MODE_LEVEL1: [ob.compress_level1(x) for x in raws], fd.MODE_RLE: [ob.compress_rle(x) for x in raws]}
    old = os.environ.get("FDH_GEN_LANES")
    try:
        for lanes in (None, "1", "8", "64"):
            if lanes is None:
                os.environ.pop("FDH_GEN_LANES", None)
            else:
                os.environ["FDH_GEN_LANES"] = lanes
            for mode in (fd.MODE_LEVEL1, fd.MODE_RLE):
                d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
                ln = fd.deflate_general_batch(d_in, d_in_off, d_out, d_out_off, mode).cpu().numpy().view(np.uint32)
                h = d_out.cpu().numpy()
                for i, raw in enumerate(raws):
                    exp = expect[mode][i]
                    got = h[out_off[i]:out_off[i] + int(ln[i])].tobytes()
                    assert got == exp, (lanes, mode, i, len(raw), int(ln[i]), len(exp))
                    assert np.all(h[out_off[i] + int(ln[i]):out_off[i + 1]] == 0x5A), (lanes, mode, i)
    finally:
        if old is None:
            os.environ.pop("FDH_GEN_LANES", None)
        else:
            os.environ["FDH_GEN_LANES"] = old


def test_general_encoder_block_longer_than_the_packed_heap_items(harness):
    """A block's Huffman merges run on one-dword heap items (22 bits of frequency) and fall back to the 64-bit items
    when the block covers 2^22 positions or more: 4.5 MiB of bytes without repeats is ONE block (a literal run counts
    as one symbol towards the 16 384 of a block) in both modes; bit-exact with the oracle, next to a short stream."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(23)
    raws = [r.integers(0, 256, 4_718_592 + 11, dtype=np.uint8).tobytes(), b"abcabcabcabc" * 50]
    buf, in_off = streams.pack_exact(raws)
    caps = [fd.compress_bound(len(x)) + 5 for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_in = torch.from_numpy(buf).cuda()
    d_in_off = torch.from_numpy(in_off.astype(np.int64)).cuda()
    d_out_off = torch.from_numpy(out_off).cuda()
    for mode, enc in ((fd.MODE_LEVEL1, ob.compress_level1), (fd.MODE_RLE, ob.compress_rle)):
        d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        ln = fd.deflate_general_batch(d_in, d_in_off, d_out, d_out_off, mode).cpu().numpy().view(np.uint32)
        h = d_out.cpu().numpy()
        for i, raw in enumerate(raws):
            exp = enc(raw)
            assert h[out_off[i]:out_off[i] + int(ln[i])].tobytes() == exp, (mode, i, int(ln[i]), len(exp))


def test_general_encoder_roundtrip_at_scale(harness):
    """8192 x 64 KiB through the level-1 and the RLE encoder on the GPU, decoded again on the GPU by
    the general kernels (dynamic blocks, real distances): every stream Ok, lengths exact, decoded ==
    raw, reported Adler-32 == the trailer the encoder wrote; the oracle byte-compares a strided
    sample of the compressed streams."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    n, L = 8192, 65536
    raw = synth.gen_batch_torch(40000, n, L)
    bound = (fd.compress_bound(L) + 15) & ~15
    in_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    c_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * bound
    for mode, enc in ((fd.MODE_LEVEL1, ob.compress_level1), (fd.MODE_RLE, ob.compress_rle)):
        comp = torch.zeros(n * bound, dtype=torch.uint8, device="cuda")
        clen = fd.deflate_general_batch(raw.view(-1), in_off, comp, c_off, mode)
        clen_h = clen.cpu().numpy().view(np.uint32)
        assert int(clen_h.max()) <= bound
        for i in range(0, n, 997):
            exp = enc(raw[i].cpu().numpy().tobytes())
            got = comp[i * bound:i * bound + int(clen_h[i])].cpu().numpy().tobytes()
            assert got == exp, (mode, i)
        out = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        out_len, status, adler = fd.inflate_batch(comp, c_off, out, in_off)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and bool((out_len == L).all()) and torch.equal(out, raw.view(-1)), mode
        idx = (c_off[:-1] + clen.to(torch.int64))[:, None] + torch.arange(-4, 0, device="cuda")[None, :]
        tr = comp[idx].to(torch.int64)
        trailer = (tr[:, 0] << 24) | (tr[:, 1] << 16) | (tr[:, 2] << 8) | tr[:, 3]
        assert torch.equal(trailer, adler.to(torch.int64) & 0xFFFFFFFF), mode
        del comp, out


@pytest.mark.parametrize("force_rccl", [False, True])
def test_multi_gpu_entry_points_every_visible_device(harness, force_rccl, monkeypatch):
    """fdh_init / fdh_inflate_batch_multi / fdh_shutdown: the mixed batch sharded by contiguous
    ranges over every visible GPU from ONE process, results all-gathered (RCCL when more than one
    device takes part, or -- second run -- forced: a one-rank communicator on a one-GPU box, so
    that ncclCommInitAll / ncclGroupStart / ncclAllGather / ncclGroupEnd of csrc/multi_gpu.cpp
    actually execute), compared stream by stream with the oracle."""
    import torch
    import fdeflate_amd as fd
    if force_rccl:
        monkeypatch.setenv("FDH_MULTI_FORCE_RCCL", "1")
    else:
        monkeypatch.delenv("FDH_MULTI_FORCE_RCCL", raising=False)
    pool = []
    for name, comp, raw in streams.valid_streams():
        pool.append((comp, len(raw)))
    for name, comp in streams.corpus_streams():
        pool.append((comp, 1 << 16))
    for item in streams.error_streams():
        pool.append((item[1], 4096))
    g = fd.init_devices(0)
    try:
        assert g == torch.cuda.device_count() >= 1
        assert fd.multi_uses_rccl() == (force_rccl or g > 1)
        if fd.multi_uses_rccl():   # librccl is mapped into this process
            assert "librccl" in open("/proc/self/maps").read()
        per = (len(pool) + g - 1) // g
        shards, expect = [], []
        for k in range(g):
            part = pool[k * per:(k + 1) * per]
            blobs = [p[0] for p in part]
            caps = [p[1] for p in part]
            buf, in_off = streams.pack_exact(blobs)
            out_off = np.zeros(len(blobs) + 1, dtype=np.int64)
            out_off[1:] = np.cumsum(np.asarray(caps, dtype=np.int64))
            dev = torch.device("cuda", k)
            shards.append((torch.from_numpy(buf).to(dev), torch.from_numpy(in_off.astype(np.int64)).to(dev),
                           torch.zeros(max(int(out_off[-1]), 1), dtype=torch.uint8, device=dev), torch.from_numpy(out_off).to(dev)))
            expect.append((harness.oracle_inflate(blobs, caps), out_off))
        results, metas = fd.inflate_batch_multi(shards)
        for k in range(g):
            (rs, rl, ra, ro), out_off = expect[k]
            ol, st, ad = (t.cpu().numpy().view(np.uint32) for t in results[k])
            h = shards[k][2].cpu().numpy()
            for i in range(len(rs)):
                assert int(st[i]) == rs[i], (k, i)
                if rs[i] in (0, 17):
                    assert int(ol[i]) == rl[i] and h[out_off[i]:out_off[i] + rl[i]].tobytes() == ro[i]
            # every device holds every shard's results
            for j in range(g):
                m = metas[j].cpu().numpy().view(np.uint32)
                assert np.array_equal(m[k, 0, :len(rs)], st) and np.array_equal(m[k, 1, :len(rs)], ol)
    finally:
        fd.shutdown_devices()


def _png_round(fd, torch, r, bpp, max_rows, wide=False):
    row_bytes = bpp * int(r.integers(1, 90)) if not wide else bpp * int(r.integers(4200 // bpp, 5000 // bpp))
    pixs, types = [], []
    for k in range(70):
        rows = int(r.integers(0, max_rows))
        pixs.append(bytes(r.integers(0, 256 if k % 3 else 4, row_bytes * rows, dtype=np.uint8)))
        types.append(bytes(r.integers(0, 5, rows, dtype=np.uint8)))
    filts = [ob.png_filter(p, row_bytes, bpp, t)[1] for p, t in zip(pixs, types)]
    pbuf, poff = streams.pack_exact(pixs)
    tbuf, toff = streams.pack_exact(types)
    fbuf, foff = streams.pack_exact(filts)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_p, d_po, d_t, d_to = d(pbuf), d(poff.astype(np.int64)), d(tbuf), d(toff.astype(np.int64))
    d_fo = d(foff.astype(np.int64))
    nf, npx = int(foff[-1]), int(poff[-1])
    d_f = torch.full((nf + 64,), 0xEE, dtype=torch.uint8, device="cuda")      # 64 guard bytes behind
    st = fd.png_filter_batch(d_p, d_po, d_t, d_to, d_f, d_fo, row_bytes, bpp)
    h = d_f.cpu().numpy()
    assert int(st.abs().sum()) == 0 and h[:nf].tobytes() == fbuf[:nf].tobytes() and np.all(h[nf:] == 0xEE)
    d_out = torch.full((npx + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    st = fd.png_unfilter_batch(d(fbuf), d_fo, d_out, d_po, row_bytes, bpp)
    h = d_out.cpu().numpy()
    assert int(st.abs().sum()) == 0 and h[:npx].tobytes() == pbuf[:npx].tobytes() and np.all(h[npx:] == 0xEE)


def test_png_filters_bit_exact_and_fused_decode(harness):
    """PNG scanline reconstruction / filtering on the GPU against the oracle's
    restatement of the PNG specification, for every pixel size, ragged image shapes from 0 rows to
    several 64-row bands, with every kernel (the pipeline over several images per wavefront, the
    default for reconstruction; one image per wavefront; one image per lane); then the fused call:
    ultra-fast streams of filtered images -> decode -> reconstruct."""
    import torch
    import fdeflate_amd as fd
    old = os.environ.get("FDH_PNG_LANE_PER_IMAGE")
    old2 = os.environ.get("FDH_PNG_NO_PIPELINE")
    old3 = os.environ.get("FDH_PNG_IMAGES_PER_WAVE")
    try:
        for per_lane, no_pipe, per_wave in (("0", "0", "1"), ("0", "0", "3"), ("0", "0", "8"), ("0", "1", "1"), ("1", "0", "1")):
            os.environ["FDH_PNG_LANE_PER_IMAGE"] = per_lane
            os.environ["FDH_PNG_NO_PIPELINE"] = no_pipe
            os.environ["FDH_PNG_IMAGES_PER_WAVE"] = per_wave
            r = np.random.default_rng(21)
            for bpp in (1, 2, 3, 4, 6, 8):
                _png_round(fd, torch, r, bpp, 12)
                _png_round(fd, torch, r, bpp, 200)
            _png_round(fd, torch, r, 4, 70, wide=True)   # rows above 4 KiB: not the pipeline's
            # a bad filter type in a later band: rows in front of it are reconstructed, status 1
            rows, rb = 150, 40
            t = np.random.default_rng(5).integers(0, 5, rows, dtype=np.uint8)
            pix = bytes(np.random.default_rng(6).integers(0, 256, rows * rb, dtype=np.uint8))
            filt = bytearray(ob.png_filter(pix, rb, 4, bytes(t))[1])
            filt[100 * (rb + 1)] = 9
            d_out = torch.zeros(rows * rb, dtype=torch.uint8, device="cuda")
            st = fd.png_unfilter_batch(torch.frombuffer(bytearray(filt), dtype=torch.uint8).cuda(),
                                       torch.tensor([0, len(filt)], dtype=torch.int64, device="cuda"), d_out,
                                       torch.tensor([0, rows * rb], dtype=torch.int64, device="cuda"), rb, 4)
            assert st.cpu().tolist() == [1] and ob.png_unfilter(bytes(filt), rb, 4)[0] == 1
            assert d_out.cpu().numpy()[:100 * rb].tobytes() == pix[:100 * rb]
    finally:
        for name, val in (("FDH_PNG_LANE_PER_IMAGE", old), ("FDH_PNG_NO_PIPELINE", old2), ("FDH_PNG_IMAGES_PER_WAVE", old3)):
            if val is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = val
    # error statuses and the fused call, with one image per wavefront and with several (an image
    # with a bad filter type, a bad size or a failed decode shares its wavefront with good ones)
    old3 = os.environ.get("FDH_PNG_IMAGES_PER_WAVE")
    try:
        for per_wave in ("1", "4", "8"):
            os.environ["FDH_PNG_IMAGES_PER_WAVE"] = per_wave
            # error statuses
            good = ob.png_filter(bytes(range(9)), 3, 1, bytes([1, 2, 4]))[1]
            bad = [good, bytes([7, 1, 2, 3]), bytes([0, 1, 2]), good, b"", good]
            bbuf, boff = streams.pack_exact(bad)
            oo = torch.from_numpy(np.arange(7, dtype=np.int64) * 16).cuda()
            pix_out = torch.full((96,), 0xEE, dtype=torch.uint8, device="cuda")
            st = fd.png_unfilter_batch(torch.from_numpy(bbuf).cuda(), torch.from_numpy(boff.astype(np.int64)).cuda(),
                                       pix_out, oo, 3, 1)
            assert st.cpu().tolist() == [0, 1, 2, 0, 0, 0]
            h = pix_out.cpu().numpy()
            for k in (0, 3, 5):
                assert h[16 * k:16 * k + 9].tobytes() == bytes(range(9)) and np.all(h[16 * k + 9:16 * k + 16] == 0xEE)
            assert np.all(h[16:48] == 0xEE) and np.all(h[64:80] == 0xEE)   # nothing written for the bad / empty ones
            # fused: 64 x 1023-byte rows with a filter byte each (the bench's buffers), RGB8, plus one broken stream
            from fdeflate_amd import synth
            n, rows, rb, bpp = 96, 64, 1023, 3
            filt_imgs = [synth.gen_stream_np(i, rows * (rb + 1)).tobytes() for i in range(n)]   # type byte 0..4 per row
            comps = [ob.compress_ultra_fast(f) for f in filt_imgs]
            comps[5] = comps[5][:-9]
            # a VALID stream that ends before its slot is full (short IDAT data): decodes fine, but
            # the rest of the slot holds stale bytes -- it must not be reconstructed (png_status 2)
            comps[9] = ob.compress_ultra_fast(filt_imgs[9][:rows * (rb + 1) - (rb + 1)])
            cbuf, coff = streams.pack_exact(comps)
            foff = np.arange(n + 1, dtype=np.int64) * (rows * (rb + 1))
            poff = np.arange(n + 1, dtype=np.int64) * (rows * rb)
            d_f = torch.zeros(int(foff[-1]), dtype=torch.uint8, device="cuda")
            d_p = torch.zeros(int(poff[-1]), dtype=torch.uint8, device="cuda")
            out_len, status, adler, pst = fd.inflate_png_batch(torch.from_numpy(cbuf).cuda(), torch.from_numpy(coff.astype(np.int64)).cuda(),
                                                               d_f, torch.from_numpy(foff).cuda(), d_p, torch.from_numpy(poff).cuda(), rb, bpp)
            torch.cuda.synchronize()
            stl, psl, hp = status.cpu().tolist(), pst.cpu().tolist(), d_p.cpu().numpy()
            for i in range(n):
                if i == 5:
                    assert stl[i] == 2 and psl[i] == 3
                    continue
                if i == 9:
                    assert stl[i] == 0 and int(out_len[i]) == (rows - 1) * (rb + 1) and psl[i] == 2
                    assert not hp[poff[i]:poff[i + 1]].any()   # nothing written
                    continue
                est, epix = ob.png_unfilter(filt_imgs[i], rb, bpp)
                assert stl[i] == 0 and psl[i] == est == 0
                assert hp[poff[i]:poff[i + 1]].tobytes() == epix, i
    finally:
        if old3 is None:
            os.environ.pop("FDH_PNG_IMAGES_PER_WAVE", None)
        else:
            os.environ["FDH_PNG_IMAGES_PER_WAVE"] = old3


@pytest.mark.gpu
def test_png_filter_fused_into_the_ultrafast_encoder():
    """fdh_png_filter_deflate_ultrafast_batch: pixel rows in, the zlib stream of the filtered image
    out, bit for bit what the oracle's filter followed by the oracle's ultra-fast encoder gives --
    every pixel size, rows shorter than a chunk, rows that are no multiple of a chunk, every
    filter type, images of one row, an empty image, a bad filter type and a size that does not fit."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(31)
    cases = []   # (pix bytes, types, row_bytes, bpp)
    for bpp in (1, 2, 3, 4, 6, 8):
        for rb in (bpp, 2 * bpp, 7 * bpp, 1023 // bpp * bpp, 40 * bpp + bpp):
            for rows in (1, 2, 5, 64):
                pix = r.integers(0, 256, rows * rb, dtype=np.uint8)
                pix[r.random(rows * rb) < 0.4] = 0
                if rows >= 5:
                    pix[rb:3 * rb] = 0       # zero rows: runs in the encoder
                types = r.integers(0, 5, rows, dtype=np.uint8)
                cases.append((pix.tobytes(), bytes(types), rb, bpp))
    for (rb, bpp) in sorted(set((c[2], c[3]) for c in cases)):
        group = [c for c in cases if c[2] == rb and c[3] == bpp]
        group.append((b"", b"", rb, bpp))                                        # an empty image
        group.append((bytes(rb * 3), bytes([0, 5, 1]), rb, bpp))                 # a bad filter type
        group.append((bytes(rb * 3 + 1) if rb > 1 else bytes(3), bytes(3), rb, bpp))   # rows do not divide / fit
        pbuf, poff = streams.pack_exact([c[0] for c in group])
        tbuf, toff = streams.pack_exact([c[1] for c in group])
        bound = [int(fd.ultrafast_bound((len(c[0]) // rb) * (rb + 1))) + 16 for c in group]
        ooff = np.zeros(len(group) + 1, dtype=np.int64)
        ooff[1:] = np.cumsum(bound)
        d_out = torch.full((int(ooff[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
        ol, st = fd.png_filter_deflate_ultrafast_batch(
            torch.from_numpy(pbuf).cuda(), torch.from_numpy(poff.astype(np.int64)).cuda(),
            torch.from_numpy(tbuf).cuda() if tbuf.size else torch.zeros(1, dtype=torch.uint8, device="cuda"),
            torch.from_numpy(toff.astype(np.int64)).cuda(), d_out, torch.from_numpy(ooff).cuda(), rb, bpp)
        torch.cuda.synchronize()
        h, oll, stl = d_out.cpu().numpy(), ol.cpu().tolist(), st.cpu().tolist()
        for i, (pix, types, _, _) in enumerate(group):
            if i == len(group) - 2:
                assert stl[i] == 1 and oll[i] == 0, (rb, bpp, i)
                continue
            if i == len(group) - 1 and rb > 1:
                assert stl[i] == 2 and oll[i] == 0, (rb, bpp, i)
                continue
            if i == len(group) - 1:
                continue
            est, filt = ob.png_filter(pix, rb, bpp, types)
            assert est == 0 and stl[i] == 0, (rb, bpp, i, stl[i])
            want = ob.compress_ultra_fast(filt)
            got = h[ooff[i]:ooff[i] + oll[i]].tobytes()
            assert got == want, (rb, bpp, i, len(got), len(want))
            assert zlib.decompress(got) == filt
            assert np.all(h[ooff[i] + oll[i]:ooff[i + 1]] == 0xEE)   # nothing behind the stream


def test_bench_through_the_distributed_path_in_a_fresh_process():
    """`bench.py --gpus 1 --force-dist` as a child process: the launcher, `init_process_group("nccl")`, the metadata
    all-gather inside the step, the barriers and the max over ranks -- the code path `--gpus 8` takes, with one rank --
    on this GPU, and one JSON line with `n_gpus`, the roofline block and a sane value at its end."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--streams", "4096",
                        "--steps", "2", "--warmup", "1", "--no-also", "--no-cpu-baseline"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["unit"] == "GB/s" and d["scaling"] == "weak"
    assert d["value"] > 50 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
