"""-m gpu: Adler-32 at its worst case.  Every kernel that computes the checksum defers the modulo and is right only while
its accumulators stay below a bound (DESIGN.md "Adler-32 accumulators"); payloads of 0xFF bytes and of bytes in
0xF8 .. 0xFF (tests/adler_payloads.py) reach those bounds, uniform random bytes reach half of them.  Decoders: every
stream of every payload through the whole pipeline, through each decoder variant and through each kernel that can run
alone -- status, length, bytes and the reported sum against the oracle and zlib.adler32.  Encoders: bit-exact against
the oracle (levels 2 and 3: tests/level_model.py), the trailer against zlib.adler32, and zlib.decompress as a third
witness.  Resume records: the Adler word of a record is the sum of the bytes in front of it, also at A = B = 65 520.

Which stream reaches which implementation (asserted as taken, not PENDING, at 65 536 bytes and more):
  inflate_seg3.h / inflate_seg2.h    the ultra-fast streams, landing decoder alone (lean and general writer) and interval
                                     kernel alone (test_kernels_alone)
  inflate_segments.h                 the ultra-fast streams, segment kernel alone: account_piece by `high`; its run form and
                                     the tail of a lane by the three sparse classes, whose zero stretches are the runs (no
                                     status tells a run from literals, so these two are reached, not asserted, beyond the
                                     streams being taken and exact)
  inflate_lanes.h                    the ultra-fast streams, lane kernel alone (it is opt-in: NO_SEGMENTS | FORCE_LANES)
  inflate_lz.h lz_flush              level-1 and zlib streams, LZ-window kernel alone
  inflate_stream.h flush_ring        flags 4 | 8 and 2 run the 12-bit kernel and nothing else: every stream up to 2^20 + 3
                                     bytes comes back Ok through flush_ring (test_every_decoder_variant allows no
                                     PENDING); 0x1000 sends the zlib streams to the tile decoders
  its twin in span_step              cannot be asserted as taken: no flag runs the span decoder alone and no status says
                                     that it ran; flags 256, 256 | 8 and 256 | 4 | 8 let it take what it takes
  the encoders                       each has an entry point of its own and no other kernel behind it
"""
import time
import zlib

import numpy as np
import pytest

import adler_payloads as ap
import level_model as lm
import oracle_binding as ob
import streams

pytestmark = pytest.mark.gpu

EMPTY = bytes.fromhex("7801030000000001")
PENDING = 0xFFFFFFFD     # and above: PENDING_RESUME, PENDING_SERIAL, PENDING -- left to a kernel that did not run
# the flag sets of test_valid_streams_every_decoder_variant, and the lane kernel (which only NO_SEGMENTS | FORCE_LANES runs)
FLAG_SETS = (8, 4 | 8, 2, 16, 16 | 8, 128, 128 | 8, 256, 256 | 8, 256 | 4 | 8, 0x400, 0x400 | 8, 0x1000, 0x1000 | 8,
             0x10000, 0x10000 | 8, 0x80000, 0x80000 | 8, 0x100000, 128 | 16, 128 | 16 | 8)
MATRIX_LENGTHS = (2049, 46764, 65537, 131073, (1 << 20) + 3)    # every flag set but 0 and 8, which see all lengths
_spent = []


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


@pytest.fixture(scope="module", autouse=True)
def _file_timed():
    t0 = time.time()
    yield
    print("tests/test_gpu_adler.py: %.1f s in all, %.1f s of it in the tests themselves" % (time.time() - t0, sum(_spent)))


@pytest.fixture(autouse=True)
def _timed(request, _file_timed):
    t0 = time.time()
    yield
    _spent.append(time.time() - t0)
    print("%s: %.1f s" % (request.node.name, _spent[-1]))


class Cases:
    """Streams of the payloads with what the oracle makes of each (decoded once per stream and shared; a slot with room
    to spare changes nothing about an Ok result)."""

    def __init__(self, harness, lengths, encodings=tuple(ap.ENCODINGS)):
        self.items = ap.cases(lengths, encodings=encodings)
        self.names = [c[0] for c in self.items]
        self.blobs = [c[1] for c in self.items]
        self.raws = [np.frombuffer(c[2], dtype=np.uint8) for c in self.items]
        rs, rl, ra, ro = harness.oracle_inflate(self.blobs, [r.size for r in self.raws])
        for name, raw, s, n, a, o in zip(self.names, self.raws, rs, rl, ra, ro):
            assert s == 0 and n == raw.size and a == zlib.adler32(raw) and o == raw.tobytes(), name
        self.sums = ra

    def run(self, harness, flags, slack=(0, 17), allow_pending=False, guard=5, align=1):
        """Every stream in a slot of its length + s for s in `slack` (rounded up to `align`).  -> names taken."""
        names = ["%s@+%d" % (n, s) for n in self.names for s in slack]
        blobs = [b for b in self.blobs for s in slack]
        raws = [r for r in self.raws for s in slack]
        sums = [a for a in self.sums for s in slack]
        caps = [-(-(r.size + s) // align) * align for r in self.raws for s in slack]
        st, ln, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags, guard=guard)
        assert guards_ok, "a kernel wrote outside its output slot (flags %#x)" % flags
        bad, taken = [], []
        for i, name in enumerate(names):
            if allow_pending and st[i] >= PENDING:
                continue
            taken.append(name)
            n = raws[i].size
            if int(st[i]) != 0:
                bad.append((name, "status", int(st[i])))
            elif int(ln[i]) != n:
                bad.append((name, "len", int(ln[i]), n))
            elif int(ad[i]) != sums[i]:
                bad.append((name, "adler", hex(int(ad[i])), hex(sums[i])))
            elif not np.array_equal(outs[i][:n], raws[i]):
                bad.append((name, "bytes", int(np.nonzero(outs[i][:n] != raws[i])[0][0])))
        assert not bad, ("flags %#x: %d of %d wrong" % (flags, len(bad), len(names)), bad[:12])
        return taken


@pytest.fixture(scope="module")
def all_cases(harness):
    return Cases(harness, ap.LENGTHS)


@pytest.fixture(scope="module")
def matrix_cases(harness):
    return Cases(harness, MATRIX_LENGTHS)


# ---- decoders ----

@pytest.mark.parametrize("flags", [0, 8], ids=hex)
def test_every_stream_whole_pipeline(harness, all_cases, flags):
    """All lengths, exact slots and slots 17 bytes loose (another alignment of every slot: gmis, and the first and last
    partial lines of every flush), the pipeline as it ships and without the serial re-check behind it."""
    all_cases.run(harness, flags)


@pytest.mark.parametrize("flags", FLAG_SETS[1:], ids=hex)
def test_every_decoder_variant(harness, matrix_cases, flags):
    """The flag sets of test_valid_streams_every_decoder_variant at the lengths 2 049, 46 764, 65 537, 131 073 and
    2^20 + 3; with NO_SEGMENTS | FORCE_LANES (the only way to the lane kernel) also in 16-byte aligned slots, the only
    ones it takes."""
    matrix_cases.run(harness, flags)
    if flags & 16 and flags & 128:
        matrix_cases.run(harness, flags, guard=16, align=16)


def _large(names, kind, encodings):
    out = []
    for n in names:
        k, length, rest = n.rsplit("_", 2)
        if k == kind and int(length) >= 65536 and rest.split("@")[0] in encodings:
            out.append(n)
    return out


# name -> (flags, 16-byte aligned slots, the format the kernel is for, payload classes it passes on as a whole)
ALONE = {
    "landing": (0x20000, False, ap.ULTRAFAST_FORMAT, ()),
    "landing_general_writer": (0x20000 | 0x80000, False, ap.ULTRAFAST_FORMAT, ()),
    "interval": (0x800, False, ap.ULTRAFAST_FORMAT, ()),            # (the landing decoder still runs in front of it)
    "interval_without_landing": (0x800 | 0x10000, False, ap.ULTRAFAST_FORMAT, ()),
    # segments_plan (inflate_segments.h) lets every lane guess a chain from the first bit of its segment and corrects a
    # wrong guess from the left neighbour, one lane further per round, for five rounds ("if (round == 5) giveup"): a
    # guess falls into step with the real chain only where the codes differ, so in a stream of one literal repeated a
    # wrong guess stays wrong in every lane behind it and the stream is left to the kernels behind -- all of `ff`
    "segment": (0x400 | 64, False, ap.ULTRAFAST_FORMAT, ("ff",)),
    "lane": (128 | 16 | 64, True, ap.ULTRAFAST_FORMAT, ()),
    "lz_window": (0x2000, False, ap.LZ_FORMAT, ()),
}


@pytest.mark.parametrize("kernel", list(ALONE))
def test_kernels_alone(harness, all_cases, kernel):
    """The kernels that can run alone: what they leave stays PENDING, everything they report is exact -- and they must not
    pass by leaving everything (the lane kernel hands a stream on when its own sum does not match the trailer: a wrong
    sum there shows ONLY as a stream that was not taken): in every payload class at least one stream of 65 536 bytes or
    more, in the format the kernel is for, is taken; a class that a documented rule of the kernel passes on is PENDING as a whole."""
    flags, aligned, fmt, passed_on = ALONE[kernel]
    taken = all_cases.run(harness, flags, allow_pending=True, guard=16 if aligned else 5, align=16 if aligned else 1)
    for kind in ap.PAYLOADS:
        large = _large(taken, kind, fmt)
        print(kernel, kind, "taken at 65 536 bytes and more:", len(large))
        if kind in passed_on:
            assert not large, (kernel, kind, "is taken after all: the rule named above no longer holds", large)
        else:
            assert large, (kernel, kind, "no stream of 65 536 bytes or more was taken")
    # `high` and `ff_sparse` at 65 536 bytes: by the landing decoder with either writer, and by the interval kernel when it
    # really is alone ("interval" is satisfied by the landing decoder in front of it)
    if kernel in ("landing", "landing_general_writer", "interval", "interval_without_landing"):
        for kind in ("high", "ff_sparse"):
            assert any(n.startswith("%s_65536_uf@" % kind) for n in taken), (kernel, kind)


def test_ordered_path_many_streams_of_high(harness):
    """Enough copies of the `high` stream of 65 536 bytes for the ordered path, through the pipeline as it ships; compared
    on the device.  fdh_launch_inflate (inflate.hip) orders a batch from n >= 4 x blocks x kS2Waves on, where blocks =
    min(ceil(n / kS2Waves), CUs) is the landing decoder's grid (s2_blocks) and kS2Waves = 16: from 64 streams per CU, 16 384
    on 256 CUs.  That grid has blocks x 16 persistent wavefronts; each decodes the stream of its own number and then
    takes further ones from a counter (inflate_seg3.hip), so with n = 64 x CUs + 16 every wavefront decodes four streams
    and more, one after the other, each from accumulators of its own.  (A batch of 4 096 is neither ordered nor does any
    wavefront of it see a second stream.)"""
    import torch
    import fdeflate_amd as fd
    waves, L = 16, 65536                                           # kS2Waves
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * cus * waves + 16
    blocks = min(-(-n // waves), cus)
    assert n >= 4 * blocks * waves, (n, cus)       # ordered, and four streams and more to each of blocks x 16 wavefronts
    raw = ap.payload("high", L)
    comp = np.frombuffer(ap.stream("high", L, "uf"), dtype=np.uint8)
    want = ap.adler32_model(raw)
    d_in = torch.cat([torch.from_numpy(comp.copy()).cuda().repeat(n), torch.zeros(256, dtype=torch.uint8, device="cuda")])
    in_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * comp.size
    out_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    d_out = torch.full((n * L + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ln, st, ad = fd.inflate_batch(d_in, in_off, d_out, out_off)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0, st[st != 0][:8].tolist()
    assert int((ln != L).sum()) == 0
    wrong = (ad != (want - (1 << 32) if want >> 31 else want)).nonzero().flatten()     # (int32 bit patterns)
    assert wrong.numel() == 0, (wrong.numel(), wrong[:8].tolist(), hex(want))
    d_raw = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    rows = d_out[:n * L].view(n, L)
    for r0 in range(0, n, 2048):                                   # (the temporaries stay small)
        assert bool((rows[r0:r0 + 2048] == d_raw).all()), r0
    assert bool((d_out[n * L:] == 0xA5).all())


# ---- encoders ----

def _check_encoded(names, raws, want, ln, slots, faults, what):
    assert not faults, (what, faults[:4])
    for name, raw, w, n, slot in zip(names, raws, want, ln, slots):
        n = int(n)
        got = slot[:n].tobytes()
        assert got == w, (what, name, n, len(w))
        assert int.from_bytes(got[-4:], "big") == zlib.adler32(raw), (what, name)
        assert zlib.decompress(got) == raw, (what, name)
        assert np.all(slot[n:] == 0x5A), (what, name, "bytes behind the stream")


def _payload_list(max_len=None):
    names, raws = [], []
    for kind in ap.PAYLOADS:
        for n in ap.LENGTHS:
            if max_len is None or n <= max_len:
                names.append("%s_%d" % (kind, n))
                raws.append(ap.payload(kind, n))
    return names, raws


def test_stored_encoder(harness):
    import fdeflate_amd as fd
    names, raws = _payload_list()
    want = [ap.stream(name.rsplit("_", 1)[0], int(name.rsplit("_", 1)[1]), "stored") for name in names]
    caps = [fd.stored_size(len(r)) + 3 for r in raws]
    ln, slots, faults = harness.gpu_encode_slots(lambda *a: fd.deflate_stored_batch(*a), raws, caps, EMPTY)
    _check_encoded(names, raws, want, ln, slots, faults, "stored")


@pytest.fixture(scope="module")
def level_model_streams():
    """Levels 2 and 3 of tests/level_model.py, up to 131 073 bytes (the model is Python)."""
    names, raws = _payload_list(131073)
    return names, raws, {level: [lm.compress(r, level) for r in raws] for level in (2, 3)}


@pytest.mark.parametrize("lanes", [None, "1", "64"])
def test_general_encoder_all_four_modes(harness, level_model_streams, lanes, monkeypatch):
    """Level 1 and RLE against the oracle at every length, levels 2 and 3 against the model up to 131 073 bytes; the
    parser with the library's own launch shape, one stream and 64 streams per wavefront."""
    import fdeflate_amd as fd
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    if lanes is not None:
        monkeypatch.setenv("FDH_GEN_LANES", lanes)
    names, raws = _payload_list()
    for mode, enc in ((fd.MODE_LEVEL1, "level1"), (fd.MODE_RLE, "rle")):
        want = [ap.stream(name.rsplit("_", 1)[0], int(name.rsplit("_", 1)[1]), enc) for name in names]
        caps = [fd.compress_bound(len(r)) + 5 for r in raws]
        ln, slots, faults = harness.gpu_encode_slots(lambda *a: fd.deflate_general_batch(*a, mode), raws, caps, EMPTY)
        _check_encoded(names, raws, want, ln, slots, faults, (enc, lanes))
    names, raws, model = level_model_streams
    for mode, level in ((fd.MODE_LEVEL2, 2), (fd.MODE_LEVEL3, 3)):
        caps = [fd.compress_bound(len(r)) + 5 for r in raws]
        ln, slots, faults = harness.gpu_encode_slots(lambda *a: fd.deflate_general_batch(*a, mode), raws, caps, EMPTY)
        _check_encoded(names, raws, model[level], ln, slots, faults, ("level%d" % level, lanes))


def test_ultrafast_encoder(harness):
    """The four payloads test_ultrafast_encode_bit_exact does not have (it has `ff` around the 256-tile fold), and `ff`
    at the lengths of this file."""
    names, raws = _payload_list()
    res, ok = harness.gpu_deflate(raws)
    assert ok, "the encoder wrote behind a stream's end"
    for name, raw, got in zip(names, raws, res):
        kind, n = name.rsplit("_", 1)
        assert got == ap.stream(kind, int(n), "uf"), (name, len(got))
        assert int.from_bytes(got[-4:], "big") == zlib.adler32(raw), name
        assert zlib.decompress(got) == raw, name


# ---- the fused PNG encoders: the checksum is over FILTERED bytes ----

def _png_images():
    """(pixels, filter types, row_bytes, bpp, PNG bit depth, colour type, width): `high` pixels under filter type 0 --
    rows of 4 095 bytes, so 32 rows are 131 072 filtered bytes, exactly the encoder's fold of 256 tiles -- and rows that
    fall by one per byte under Sub: every filtered byte but the type bytes is 0xFF."""
    out = []
    for rows in (31, 32, 33):
        out.append((ap.payload("high", rows * 4095), bytes(rows), 4095, 3, 8, 2, 1365))
    falling = ((0xFF - np.arange(4095)) & 0xFF).astype(np.uint8).tobytes()
    for rows in (31, 32, 33):
        out.append((falling * rows, bytes([1]) * rows, 4095, 1, 8, 0, 4095))
    return out


def _png_expect(pix, types, rb, bpp):
    est, filt = ob.png_filter(pix, rb, bpp, types)
    assert est == 0
    return filt, ob.compress_ultra_fast(filt)


def _check_png(h, ooff, oll, stl, want, what):
    for i, (filt, w) in enumerate(want):
        assert stl[i] == 0, (what, i, stl[i])
        got = h[ooff[i]:ooff[i] + oll[i]].tobytes()
        assert got == w, (what, i, len(got), len(w))
        assert int.from_bytes(got[-4:], "big") == zlib.adler32(filt), (what, i)
        assert zlib.decompress(got) == filt, (what, i)
        assert np.all(h[ooff[i] + oll[i]:ooff[i + 1]] == 0xEE), (what, i)


def test_png_fused_encoder_heavy_filtered_bytes(harness):
    import torch
    import fdeflate_amd as fd
    images = _png_images()
    filt = _png_expect(*images[3][:4])[0]
    assert filt.count(b"\xff") == len(filt) - 31      # the falling rows under Sub: all 0xFF but the 31 type bytes
    for group in (images[:3], images[3:]):
        rb, bpp = group[0][2], group[0][3]
        want = [_png_expect(*g[:4]) for g in group]
        pbuf, poff = streams.pack_exact([g[0] for g in group])
        tbuf, toff = streams.pack_exact([g[1] for g in group])
        ooff = np.zeros(len(group) + 1, dtype=np.int64)
        ooff[1:] = np.cumsum([int(fd.ultrafast_bound(len(f))) + 16 for f, _ in want])
        d_out = torch.full((int(ooff[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
        ol, st = fd.png_filter_deflate_ultrafast_batch(
            torch.from_numpy(pbuf).cuda(), torch.from_numpy(poff.astype(np.int64)).cuda(), torch.from_numpy(tbuf).cuda(),
            torch.from_numpy(toff.astype(np.int64)).cuda(), d_out, torch.from_numpy(ooff).cuda(), rb, bpp)
        torch.cuda.synchronize()
        _check_png(d_out.cpu().numpy(), ooff, ol.cpu().tolist(), st.cpu().tolist(), want, ("uniform", rb, bpp))


def test_png_fused_mixed_encoder_heavy_filtered_bytes(harness):
    """The same images in one mixed batch, next to a 5 x 3 one."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(53)
    images = _png_images()
    images.insert(3, (r.integers(0, 256, 15, dtype=np.uint8).tobytes(), bytes([0, 1, 2]), 5, 1, 8, 0, 5))
    want = [_png_expect(*g[:4]) for g in images]
    pbuf, poff = streams.pack_exact([g[0] for g in images])
    tbuf, toff = streams.pack_exact([g[1] for g in images])
    ooff = np.zeros(len(images) + 1, dtype=np.int64)
    ooff[1:] = np.cumsum([int(fd.ultrafast_bound(len(f))) + 16 for f, _ in want])
    width = torch.tensor([g[6] for g in images], dtype=torch.int32, device="cuda")
    height = torch.tensor([len(g[1]) for g in images], dtype=torch.int32, device="cuda")
    pairs = torch.tensor([[g[4], g[5]] for g in images], dtype=torch.int32, device="cuda")
    info = fd.png_encode_records(width, height, pairs)
    d_out = torch.full((int(ooff[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
    ol, st = fd.png_filter_deflate_ultrafast_mixed_batch(
        torch.from_numpy(pbuf).cuda(), torch.from_numpy(poff.astype(np.int64)).cuda(), torch.from_numpy(tbuf).cuda(),
        torch.from_numpy(toff.astype(np.int64)).cuda(), d_out, torch.from_numpy(ooff).cuda(), info)
    torch.cuda.synchronize()
    _check_png(d_out.cpu().numpy(), ooff, ol.cpu().tolist(), st.cpu().tolist(), want, "mixed")


# ---- resume records ----

class Resumed:
    """One stream through fdh_inflate_batch_resumable, call by call, in one slot that stays where it is."""

    def __init__(self, fd, comp, cap, flags):
        import torch
        self.fd, self.comp, self.cap, self.flags = fd, comp, cap, flags
        self.out = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        self.rec = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        self.calls = 0

    def call(self, in_len, room):
        """-> (status, out_len, adler, record as four uint32)"""
        import torch
        d_in = torch.from_numpy(np.frombuffer(self.comp[:in_len] + bytes(16), dtype=np.uint8).copy()).cuda()
        io = torch.tensor([0, in_len], dtype=torch.int64, device="cuda")
        oo = torch.tensor([0, room], dtype=torch.int64, device="cuda")
        ln, st, ad = self.fd.inflate_batch_resumable(d_in, io, self.out, oo, self.rec, flags=self.flags, resume_in=self.calls > 0)
        torch.cuda.synchronize()
        self.calls += 1
        u = lambda t: int(t.cpu().numpy().view(np.uint32)[0])
        return u(st), u(ln), u(ad), [int(x) for x in self.rec.cpu().numpy().view(np.uint32)[0]]

    def host(self):
        return self.out.cpu().numpy()


def _record_is_sum_of_prefix(r, rec, produced, raw):
    """The record's Adler word is the Adler-32 of the bytes in front of the place it names, which are in the slot."""
    opos = rec[2]
    assert opos <= produced, (rec, produced)
    assert r.host()[:opos].tobytes() == raw[:opos]
    assert rec[3] == ap.adler32_model(raw[:opos]) == zlib.adler32(raw[:opos]), (rec, hex(zlib.adler32(raw[:opos])))


def _finish(r, raw):
    st, ln, ad, rec = r.call(len(r.comp), len(raw))
    assert (st, ln) == (0, len(raw)) and ad == zlib.adler32(raw), (st, ln, hex(ad))
    assert not any(rec), rec
    h = r.host()
    assert h[:len(raw)].tobytes() == raw and np.all(h[len(raw):] == 0xA5)


def _stored_with_a_block_end_at(raw, at):
    """A stored-block zlib stream of `raw` with one block ending exactly at byte `at`."""
    cuts = list(range(0, at, 65535)) + list(range(at, len(raw), 65535)) + [len(raw)]
    out = bytearray(b"\x78\x01")
    for k in range(len(cuts) - 1):
        n = cuts[k + 1] - cuts[k]
        out += bytes([1 if k == len(cuts) - 2 else 0]) + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + raw[cuts[k]:cuts[k + 1]]
    return bytes(out) + zlib.adler32(raw).to_bytes(4, "big")


@pytest.mark.parametrize("flags", [0, 0x1000], ids=hex)
@pytest.mark.parametrize("encoding", ["huff", "stored"])
def test_resume_from_the_largest_state(harness, encoding, flags):
    """200 000 bytes of 0xFF as one-byte tokens (Huffman-only, stored), stopped by a slot of 46 764 and of 112 285 bytes:
    there A = B = 65 520, and the call that takes the stream up again starts its sums from the largest state there is
    -- in the LZ-window kernel and, with 0x1000, in the 12-bit kernel.  Then stopped by the end of the input instead.
    Every record's Adler word is the sum of the prefix it names.
    By design a record lies where decoding can start again, not where the room ended: a few literals early (three
    and six bytes here) and, in a stored block, at the block's header.  The record AT the largest state
    is therefore, Huffman-only, the kernel's own record moved on by hand over the literals between (a bit each: the
    code has two symbols) and, stored, the kernel's own record of a stream whose block ends right there."""
    import fdeflate_amd as fd
    raw = ap.payload("ff", 200000)
    comp = ap.ENCODINGS[encoding](raw)
    for room in ap.MAXIMAL_STATE_LENGTHS:
        r = Resumed(fd, comp, len(raw), flags)
        st, ln, ad, rec = r.call(len(comp), room)
        assert (st, ln) == (17, room), (st, ln)
        print(encoding, hex(flags), "room", room, "record", [hex(x) for x in rec])
        _record_is_sum_of_prefix(r, rec, room, raw)
        _finish(r, raw)
        if encoding == "huff":
            r = Resumed(fd, comp, len(raw), flags)
            st, ln, ad, rec = r.call(len(comp), room)
            assert 0 < rec[2] <= room and room - rec[2] < 16, rec
            moved = [rec[0], rec[1] + (room - rec[2]), room, 0xFFF0FFF0]
            r.rec.copy_(r.rec.new_tensor(np.array([moved], dtype=np.uint32).view(np.int32)))
            _finish(r, raw)
        else:
            blocks = _stored_with_a_block_end_at(raw, room)
            assert zlib.decompress(blocks) == raw
            r = Resumed(fd, blocks, len(raw), flags)
            st, ln, ad, rec = r.call(len(blocks), room + 1000)
            assert (st, ln) == (17, room + 1000), (st, ln)
            print(encoding, hex(flags), "block end", room, "record", [hex(x) for x in rec])
            assert rec[2] == room and rec[3] == 0xFFF0FFF0, [hex(x) for x in rec]
            _finish(r, raw)
    # the input cut: in the stored stream right behind byte 46 764 / 112 285 of the payload, in the Huffman-only one
    # (a bit per byte) as near as a byte boundary comes
    for target in ap.MAXIMAL_STATE_LENGTHS:
        if encoding == "stored":
            cut = 2 + 5 * (target // 65535 + 1) + target
        else:
            cut = len(comp) - 4 - (len(raw) - target) // 8
        r = Resumed(fd, comp, len(raw), flags)
        st, ln, ad, rec = r.call(cut, len(raw))
        d = ob.Decompressor()
        buf = np.zeros(len(raw), dtype=np.uint8)
        _, _, produced = d.read(comp[:cut], buf, 0)
        assert (st, ln) == (2, produced), (st, ln, produced)
        print(encoding, hex(flags), "cut", cut, "produced", produced, "record", [hex(x) for x in rec])
        _record_is_sum_of_prefix(r, rec, produced, raw)
        _finish(r, raw)


def test_streaming_huffman_only_ff_through_a_small_window(harness):
    """Decompressor.read over the Huffman-only stream of 2^20 + 3 bytes of 0xFF, the input in pieces of 64 KiB, the output
    through a 32 KiB window behind 32 KiB of history: the bytes of the oracle's streaming decoder driven the same way,
    done at the end, no WrongChecksum on the way."""
    import fdeflate_amd as fd
    raw = ap.payload("ff", (1 << 20) + 3)
    comp = ap.stream("ff", (1 << 20) + 3, "huff")

    def drain(read, is_done):
        got = bytearray()
        buf = np.zeros(65536, dtype=np.uint8)
        pos = k = calls = 0
        have = 65536
        while not is_done():
            calls += 1
            assert calls < 5000
            c, p = read(comp[k:min(have, len(comp))], buf, pos)
            k += c
            got += buf[pos:pos + p].tobytes()
            pos += p
            if p == 0 and c == 0:
                assert have < len(comp), "no progress with the whole input at hand"
                have += 65536
            if pos > 32768:
                buf[:32768] = buf[pos - 32768:pos].copy()
                pos = 32768
        return bytes(got)

    d = fd.Decompressor()
    got = drain(d.read, d.is_done)          # (raises DecompressionError on any status but Ok)
    assert d.is_done()
    o = ob.Decompressor()

    def oracle_read(data, buf, pos):
        st, c, p = o.read(data, buf, pos)
        assert st == 0, st
        return c, p
    want = drain(oracle_read, o.is_done)
    assert o.is_done() and want == raw
    assert got == want
