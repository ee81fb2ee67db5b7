"""-m gpu: long inputs in pieces (include/fdeflate_hip_pieces.h, fdeflate_amd.pieces).

Piece mode of the block writer alone, the stitch kernels alone on synthetic pieces, deflate_level_pieces_batch end to
end, and the three PNG pipelines.  The expected bytes are tests/pieces_model.py's (tests/test_pieces_model.py checks
those on the CPU); every buffer a kernel writes to is compared as a whole, guard bytes included.
"""
import functools
import zlib

import numpy as np
import pytest

import adler_payloads
import pieces_model as pm
import png_corpus as pc
import png_gpu_harness as gh
import png_levels_cases as lc

pytestmark = pytest.mark.gpu

GUARD = gh.GUARD
SLICE_LENGTHS = (0, 1, 3, 4, 7, 8, 63, 64, 65, 257, 4096)


def _text(n, seed=15100, vocabulary=40, letters=4):
    """Words with a few odd bytes between them: matches at every level.  (A large vocabulary over many letters keeps the
    hash chains short, and with them the time the lazy models take.)"""
    r = np.random.default_rng(seed)
    words = [bytes(r.integers(97, 97 + letters, int(r.integers(3, 9)), dtype=np.uint8)) for _ in range(vocabulary)]
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(0, vocabulary))] + (b" " if r.integers(0, 8) else bytes(r.integers(0, 256, 2, dtype=np.uint8)))
    return bytes(out[:n])


def _long_text(n, seed):
    """_text(50 000) over and over with one byte in 200 replaced: long inputs without a Python loop over their words."""
    base = np.frombuffer(_text(50000, seed, 4000, 26), dtype=np.uint8)
    out = np.tile(base, (n + base.size - 1) // base.size)[:n].copy()
    r = np.random.default_rng(seed + 1)
    at = r.integers(0, max(n, 1), n // 200)
    out[at] = r.integers(0, 256, at.size, dtype=np.uint8)
    return out.tobytes()


def _as_bytes(t, a, b):
    return t[a:b].tobytes()


# ---- piece mode alone ----

@functools.lru_cache(maxsize=None)
def _small_pieces(level):
    """[(slice, last, expected piece)]: every slice length as a last and as a non-last piece."""
    text = _text(8192)
    out = []
    for k, n in enumerate(SLICE_LENGTHS):
        for last in (True, False):
            data = text[17 * k:17 * k + n]
            out.append((data, last, pm.piece(data, level, last)))
    return out


def _run_pieces(pcs, level, items, short=()):
    """One launch over `items` [(slice, last, expected)]: slots of compress_bound between guard bytes -- `short`: the
    indices whose slot is one byte under the piece -- and the whole output buffer compared.  -> nothing; asserts."""
    import torch
    import fdeflate_amd as fd
    raw = b"".join(d for d, _, _ in items)
    p_off = gh.offsets([len(d) for d, _, _ in items])
    sizes = [len(e) - 1 if k in short else fd.compress_bound(len(d)) for k, (d, _, e) in enumerate(items)]
    o_off = gh.offsets(sizes, front=5)
    out = torch.full((int(o_off[-1]) + 9,), GUARD, dtype=torch.uint8, device="cuda")
    d_raw = gh.dev(np.frombuffer(raw or b"\0", dtype=np.uint8))
    last = gh.dev(np.array([3 if l else 0 for _, l, _ in items], dtype=np.uint8))       # (any non-zero byte is "last")
    got_len, got_adler = pcs.deflate_level_pieces_raw_batch(d_raw, gh.dev(p_off), last, out, gh.dev(o_off), level)
    torch.cuda.synchronize()
    got_len, got_adler, host = got_len.cpu().tolist(), got_adler.cpu().numpy().view(np.uint32).tolist(), out.cpu().numpy()
    want = np.full(host.size, GUARD, dtype=np.uint8)
    for k, (d, _, e) in enumerate(items):
        if k in short:
            assert got_len[k] == -1, k
            want[o_off[k]:o_off[k + 1]] = host[o_off[k]:o_off[k + 1]]       # (what a slot that is too small holds is not defined)
            continue
        assert got_len[k] == len(e), (k, len(d), got_len[k], len(e))
        assert got_adler[k] == zlib.adler32(d), (k, len(d))
        want[o_off[k]:o_off[k] + len(e)] = np.frombuffer(e, dtype=np.uint8)
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, "first differing byte at %d (slots from %s)" % (bad[0], o_off[:4].tolist())


@pytest.mark.parametrize("level", [1, 3, 4, 6, 9])
def test_piece_mode_against_the_model(level):
    """Every slice length as a last and a non-last piece, 1, 8 and 64 pieces per launch; in the launch of 64 also the
    pinned inputs whose non-last piece has two blocks, both ways, and a slot one byte short."""
    import fdeflate_amd.pieces as pcs
    small = _small_pieces(level)
    for per_launch in (1, 8):
        for k in range(0, len(small), per_launch):
            _run_pieces(pcs, level, small[k:k + per_launch])
    data, non_last, last, blocks = pm.two_block_pieces(level)
    assert blocks == pm.TWO_BLOCK[level][1]
    items = small + [(data, False, non_last), (data, True, last)] + small
    items = (items + small)[:64]
    assert len(items) == 64
    _run_pieces(pcs, level, items, short=(9, len(small)))                   # a 7-byte slice, and the two-block non-last piece


# ---- stitch alone ----

PIECE_LENGTHS = tuple(range(1, 71)) + (4095, 4096, 4097)
PIECE_COUNTS = (1, 2, 3, 64, 65, 1000)
RAW_SIZES = (64, 5552, 65521, 65536)


@functools.lru_cache(maxsize=None)
def _synthetic():
    """Inputs of PIECE_COUNTS pieces (and two that must fail) whose "compressed" pieces are random bytes of PIECE_LENGTHS
    in turn, their raw bytes 0xFF payloads cut at RAW_SIZES in turn.  -> per input (pieces, raw sizes, checksums)."""
    r = np.random.default_rng(15200)
    inputs, at = [], 0
    for count in PIECE_COUNTS + (3, 2):
        pieces = [bytes(r.integers(0, 256, PIECE_LENGTHS[(at + j) % len(PIECE_LENGTHS)], dtype=np.uint8)) for j in range(count)]
        raw_sizes = [RAW_SIZES[(at + j) % 4] - (j % 3) for j in range(count)]
        at += count
        whole = adler_payloads.ff(sum(raw_sizes))
        adlers, o = [], 0
        for n in raw_sizes:
            adlers.append(zlib.adler32(whole[o:o + n]))
            o += n
        inputs.append((pieces, raw_sizes, adlers, zlib.adler32(whole)))
    return inputs


def test_stitch_on_synthetic_pieces():
    """Piece lengths 1 .. 70 and 4 095 .. 4 097 at every source and destination alignment, inputs of 1 .. 1 000 pieces,
    one with a failed piece among good ones and one whose total is a byte over its slot: whole buffers, guards on both
    sides of every slot, the combined checksum zlib's of the 0xFF payload."""
    import torch
    import fdeflate_amd.pieces as pcs
    inputs = _synthetic()
    n = len(inputs)
    failed_input, tight_input = n - 2, n - 1
    pieces = [p for inp in inputs for p in inp[0]]
    total = len(pieces)
    # piece k's slot starts k % 16 bytes past a 16-byte boundary and ends 1 .. 16 bytes behind the piece
    slot_off = np.zeros(total + 1, dtype=np.int64)
    at = 0
    for k, p in enumerate(pieces):
        at += (k % 16 - at) % 16
        slot_off[k] = at
        at += len(p) + 1
    slot_off[total] = at
    scratch = np.full(at + 16, GUARD, dtype=np.uint8)
    for k, p in enumerate(pieces):
        scratch[slot_off[k]:slot_off[k] + len(p)] = np.frombuffer(p, dtype=np.uint8)
    piece_len = np.array([len(p) for p in pieces], dtype=np.int32)
    first = gh.offsets([len(inp[0]) for inp in inputs])
    piece_len[first[failed_input] + 1] = -1
    piece_off = gh.offsets([s for inp in inputs for s in inp[1]], front=11)
    adler = np.array([a for inp in inputs for a in inp[2]], dtype=np.uint32)
    streams = [pm.stitch(inp[0], b"")[:-4] + inp[3].to_bytes(4, "big") for inp in inputs]
    # every out slot: 3 guard bytes in front (inside the slot in front of it), the stream, 4 spare bytes; the tight one a byte short
    sizes = [len(s) + 7 for s in streams]
    sizes[tight_input] = len(streams[tight_input]) - 1
    out_off = gh.offsets(sizes, front=13)
    out = torch.full((int(out_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    d_scratch, d_adler = gh.dev(scratch), gh.dev(adler.view(np.int32))
    src_align = {(d_scratch.data_ptr() + int(o)) % 16 for o in slot_off[:total]}
    got = pcs.deflate_stitch_batch(d_scratch, gh.dev(slot_off), gh.dev(piece_len), d_adler, gh.dev(piece_off), gh.dev(first), out, gh.dev(out_off))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    want = np.full(host.size, GUARD, dtype=np.uint8)
    want_len, dst_align = [], set()
    for i, s in enumerate(streams):
        if i in (failed_input, tight_input):
            want_len.append(-1)
            continue
        want_len.append(len(s))
        want[out_off[i]:out_off[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
        o = out.data_ptr() + int(out_off[i]) + 2
        for p in inputs[i][0]:
            dst_align.add(o % 16)
            o += len(p)
    assert src_align == set(range(16)) == dst_align
    assert got.cpu().tolist() == want_len
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, "first differing byte at %d" % bad[0]
    assert np.array_equal(d_scratch.cpu().numpy(), scratch)                 # the source is read only
    # the scratch the call leaves in piece_adler: every piece's place in its stream, -1 for a failed input's
    places = d_adler.cpu().numpy().view(np.uint32)
    for i in range(n):
        exp = [0xFFFFFFFF] * len(inputs[i][0]) if want_len[i] < 0 else (2 + np.cumsum([0] + [len(p) for p in inputs[i][0]][:-1])).tolist()
        assert places[first[i]:first[i + 1]].tolist() == exp, i


# ---- end to end ----

def _sizes(piece_bytes):
    return (0, piece_bytes // 2 + 1, piece_bytes, piece_bytes + 1, 2 * piece_bytes + 7, 300 * piece_bytes - 5)


MODEL_BYTES = 1300000   # inputs up to this size are compared with the model's stream whole: all but the 19.6 MB one


@functools.lru_cache(maxsize=None)
def _expected(level, piece_bytes):
    """Per input (data, whole stream or None, the model's first two pieces, its last two pieces)."""
    text = _long_text(300 * piece_bytes, 15300)
    out = []
    for n in _sizes(piece_bytes):
        data = text[:n]
        if n <= MODEL_BYTES:
            out.append((data, pm.compress(data, level, piece_bytes), None, None))
        else:
            spans = pm.cuts(n, piece_bytes)
            head = b"".join(pm.piece(data[s:e], level, False) for s, e in spans[:2])
            tail = pm.piece(data[spans[-2][0]:spans[-2][1]], level, False) + pm.piece(data[spans[-1][0]:], level, True)
            out.append((data, None, head, tail))
    return out


@pytest.mark.parametrize("piece_bytes", [64, 1000, 4096, 65536])
@pytest.mark.parametrize("level", [1, 3, 6, 9])
def test_end_to_end_against_the_model_zlib_and_the_decoder(level, piece_bytes):
    """Inputs of one (empty), one, one (full), two, three and 300 pieces in one call: the model's stitched bytes (but for
    the 300 pieces of 65 536 bytes, 19.6 MB, which the Python models take about two minutes for at level 6: there the
    model's first two and last two pieces around a middle that zlib and the device decoder vouch for), guards around the slots, zlib and fd.inflate_batch give the
    inputs back, and an input of at most piece_bytes is levels.deflate_level_batch's stream."""
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.levels as lv
    import fdeflate_amd.pieces as pcs
    cases = _expected(level, piece_bytes)
    datas = [c[0] for c in cases]
    raw = gh.dev(np.frombuffer(b"".join(datas), dtype=np.uint8))
    in_off = gh.dev(gh.offsets([len(d) for d in datas]))
    bounds = [pcs.pieces_bound(len(d), level, piece_bytes) for d in datas]
    o_off = gh.offsets(bounds, front=41)
    out = torch.full((int(o_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    got = pcs.deflate_level_pieces_batch(raw, in_off, out, gh.dev(o_off), level, piece_bytes)
    torch.cuda.synchronize()
    lens, host = got.cpu().tolist(), out.cpu().numpy()
    assert (host[:41] == GUARD).all() and (host[o_off[-1]:] == GUARD).all()
    for k, (data, whole, head, tail) in enumerate(cases):
        assert 0 < lens[k] <= bounds[k], (k, lens[k])
        stream = _as_bytes(host, o_off[k], o_off[k] + lens[k])
        assert (host[o_off[k] + lens[k]:o_off[k + 1]] == GUARD).all(), k
        if whole is not None:
            assert stream == whole, (k, len(data))
        else:
            assert stream[:2 + len(head)] == b"\x78\x01" + head, k
            assert stream[-4 - len(tail):] == tail + zlib.adler32(data).to_bytes(4, "big"), k
        assert zlib.decompress(stream) == data, k
    # the device decoder
    r_off = gh.dev(gh.offsets([len(d) for d in datas]))
    back = torch.full((max(1, sum(len(d) for d in datas)),), GUARD, dtype=torch.uint8, device="cuda")
    b_len, status, adler = fd.inflate_batch(out, gh.dev(o_off), back, r_off)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(datas) and b_len.cpu().tolist() == [len(d) for d in datas]
    assert back.cpu().numpy()[:raw.numel()].tobytes() == b"".join(datas)
    assert adler.cpu().numpy().view(np.uint32).tolist() == [zlib.adler32(d) for d in datas]
    # one piece: the whole-stream encoder's bytes
    ks = [k for k, d in enumerate(datas) if len(d) <= piece_bytes]
    one = b"".join(datas[k] for k in ks)
    w_off = gh.offsets([fd.compress_bound(len(datas[k])) for k in ks])
    w_out = torch.full((int(w_off[-1]),), GUARD, dtype=torch.uint8, device="cuda")
    w_len = lv.deflate_level_batch(gh.dev(np.frombuffer(one, dtype=np.uint8)), gh.dev(gh.offsets([len(datas[k]) for k in ks])), w_out,
                                   gh.dev(w_off), level)
    torch.cuda.synchronize()
    w_len, w_host = w_len.cpu().tolist(), w_out.cpu().numpy()
    assert len(ks) == 3
    for j, k in enumerate(ks):
        assert _as_bytes(w_host, w_off[j], w_off[j] + w_len[j]) == _as_bytes(host, o_off[k], o_off[k] + lens[k]), k


def test_end_to_end_slots_one_byte_short_level_0_and_the_one_shot():
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.levels as lv
    import fdeflate_amd.pieces as pcs
    datas = [_text(n, seed=15400) for n in (0, 300, 1000)]
    raw, in_off = gh.dev(np.frombuffer(b"".join(datas), dtype=np.uint8)), gh.dev(gh.offsets([len(d) for d in datas]))
    want = [pm.compress(d, 6, 64) for d in datas]
    sizes = [len(want[0]), len(want[1]) - 1, len(want[2])]
    o_off = gh.offsets(sizes, front=3)
    out = torch.full((int(o_off[-1]) + 5,), GUARD, dtype=torch.uint8, device="cuda")
    got = pcs.deflate_level_pieces_batch(raw, in_off, out, gh.dev(o_off), 6, 64)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [len(want[0]), -1, len(want[2])]
    exp = np.frombuffer(bytes([GUARD]) * 3 + want[0] + bytes([GUARD]) * sizes[1] + want[2] + bytes([GUARD]) * 5, dtype=np.uint8)
    assert np.array_equal(out.cpu().numpy(), exp)
    # level 0 goes down the existing route
    o_off = gh.offsets([fd.stored_size(len(d)) for d in datas])
    a = torch.full((int(o_off[-1]),), GUARD, dtype=torch.uint8, device="cuda")
    b = a.clone()
    la, lb = pcs.deflate_level_pieces_batch(raw, in_off, a, gh.dev(o_off), 0, 64), lv.deflate_level_batch(raw, in_off, b, gh.dev(o_off), 0)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(la, lb)
    for level in (1, 4, 9):
        assert pcs.compress_to_vec_level_pieces(datas[2], level, 64) == pm.compress(datas[2], level, 64)
        assert pcs.compress_to_vec_level_pieces(datas[2], level) == lv.compress_to_vec_with_level(datas[2], level)
    assert pcs.compress_to_vec_level_pieces(b"", 6, 64) == b"\x78\x01\x03\x00\x00\x00\x00\x01"
    assert pcs.compress_to_vec_level_pieces(datas[1], 0, 64) == lv.compress_to_vec_with_level(datas[1], 0)


def test_one_read_back_beyond_the_encoders(monkeypatch):
    """deflate_level_pieces_batch moves eight bytes from the device to the host: the number of pieces."""
    import torch
    import fdeflate_amd.pieces as pcs
    from fdeflate_amd import api
    seen = []
    real = api._read_back
    monkeypatch.setattr(api, "_read_back", lambda t: seen.append(t.numel() * t.element_size()) or real(t))
    datas = [_text(n, seed=15500) for n in (500, 0, 129)]
    raw, in_off = gh.dev(np.frombuffer(b"".join(datas), dtype=np.uint8)), gh.dev(gh.offsets([len(d) for d in datas]))
    o_off = gh.offsets([pcs.pieces_bound(len(d), 3, 64) for d in datas])
    out = torch.empty(int(o_off[-1]), dtype=torch.uint8, device="cuda")
    got = pcs.deflate_level_pieces_batch(raw, in_off, out, gh.dev(o_off), 3, 64)
    assert seen == [8]
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for k, d in enumerate(datas):
        assert _as_bytes(host, o_off[k], o_off[k] + int(got[k])) == pm.compress(d, 3, 64)


# ---- PNG ----

def _collection(cases):
    import torch
    bufs = [np.ascontiguousarray(c[1]).view(np.uint8).reshape(-1) for c in cases]
    off = gh.offsets([b.size for b in bufs])
    pairs = torch.tensor([list(c[4] or (0, 0)) for c in cases], dtype=torch.int32, device="cuda")
    return gh.dev(np.concatenate(bufs)), gh.dev(off), gh.words([c[2] for c in cases]), gh.words([c[3] for c in cases]), pairs


def _files(file, f_off, f_len):
    host, offs, lens = file.cpu().numpy(), f_off.cpu().tolist(), f_len.cpu().tolist()
    return [host[offs[k]:offs[k] + lens[k]].tobytes() for k in range(len(lens))]


def _in_pieces(f, level, piece_bytes):
    """The file `f` of the whole-stream pipeline with its IDAT payload encoded in pieces instead."""
    import png_file_model as fm
    idat = lc.idat_of(f)
    at = f.index(b"IDAT") - 4
    assert f[at + 12 + len(idat):at + 20 + len(idat)] == b"\0\0\0\0IEND"      # (one IDAT chunk)
    return f[:at] + fm.chunk(b"IDAT", pm.compress(lc.inflate(idat), level, piece_bytes), crc=zlib.crc32) + f[at + 12 + len(idat):]


@pytest.mark.parametrize("piece_bytes", [64, 1000, 65536])
@pytest.mark.parametrize("level", [1, 4, 6, 9])
def test_rgba8_pipeline_in_pieces(level, piece_bytes):
    """The case pictures (up to 5 800 filtered bytes, two failing ones among them) in one mixed batch: every file is the
    whole-stream pipeline's with its IDAT payload replaced by the model's stitched stream -- at 65 536, above every
    filtered size, the same file byte for byte -- and decodes back in Pillow and on the device."""
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.pieces as pcs
    cases, expected = lc.cases8(), lc.expected8(level)
    rgba, r_off, width, height, pairs = _collection(cases)
    file, f_off, f_len, st, info = pcs.png_encode_mixed_rgba_files_level_pieces_batch(rgba, r_off, width, height, level, pairs=pairs,
                                                                                     piece_bytes=piece_bytes)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [e[0] for e in expected]
    files = _files(file, f_off, f_len)
    for k, (e_st, want, depth, colour) in enumerate(expected):
        if e_st:
            assert files[k] == b"", cases[k][0]
            continue
        assert files[k] == (want if piece_bytes == 65536 else _in_pieces(want, level, piece_bytes)), cases[k][0]
        assert pc.pillow_rgba(files[k]) == cases[k][1].tobytes(), cases[k][0]
    good = [k for k, f in enumerate(files) if f]
    host, offs, lens = gh.batch_of([files[k] for k in good])
    back, back_off, _, status, png_status = fd.png_decode_mixed_files_rgba_batch(gh.dev(host), gh.dev(offs), file_len=gh.dev(lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(good) and png_status.cpu().tolist() == [0] * len(good)
    back, back_off = back.cpu().numpy(), back_off.cpu().tolist()
    for j, k in enumerate(good):
        assert back[back_off[j]:back_off[j + 1]].tobytes() == cases[k][1].tobytes(), cases[k][0]


@pytest.mark.parametrize("piece_bytes", [64, 1000, 65536])
@pytest.mark.parametrize("level", [1, 6])
def test_rgba16_pipeline_in_pieces(level, piece_bytes):
    import torch
    import fdeflate_amd.pieces as pcs
    import png16_encode_cases as c16
    from fdeflate_amd import png16
    cases, expected = lc.cases16(), lc.expected16(level)
    rgba16, r_off, width, height, pairs = _collection(cases)
    file, f_off, f_len, st, _ = pcs.png_encode_mixed_rgba16_files_level_pieces_batch(rgba16, r_off, width, height, level, pairs=pairs,
                                                                                    piece_bytes=piece_bytes)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [e[0] for e in expected]
    files = _files(file, f_off, f_len)
    for k, (e_st, want, depth, colour) in enumerate(expected):
        if e_st:
            assert files[k] == b"", cases[k][0]
            continue
        assert files[k] == (want if piece_bytes == 65536 else _in_pieces(want, level, piece_bytes)), cases[k][0]
        c16.check_in_pillow(files[k], cases[k][1], cases[k][2], cases[k][3], depth, colour)
    good = [k for k, f in enumerate(files) if f]
    host, offs, lens = gh.batch_of([files[k] for k in good], front=6, slack=2)
    back, back_off, _, status, png_status = png16.png_decode_mixed_files_rgba16_batch(gh.dev(host), gh.dev(offs), file_len=gh.dev(lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(good) and png_status.cpu().tolist() == [0] * len(good)
    back, back_off = back.cpu().numpy(), back_off.cpu().tolist()
    for j, k in enumerate(good):
        assert back[back_off[j]:back_off[j + 1]].tobytes() == cases[k][1].tobytes(), cases[k][0]


@pytest.mark.parametrize("piece_bytes", [64, 1000, 65536])
@pytest.mark.parametrize("level", [0, 3, 6])
def test_packed_scanlines_pipeline_in_pieces(level, piece_bytes):
    """png_encode_mixed_files_level_pieces_batch on the packed scanlines of the good pictures that need no palette, and a
    dimension record among them (status 3, no file); level 0 goes down the existing route."""
    import torch
    import fdeflate_amd.pieces as pcs
    import png_mixed_model as mm
    import png_pack_model as ppm
    cases, expected = lc.cases8(), lc.expected8(level)
    ks = [k for k, e in enumerate(expected) if e[0] == 0 and e[3] != 3]
    packed, records = [], []
    for k in ks:
        _, px, w, h, _, _ = cases[k]
        depth, colour = expected[k][2:]
        pix, st = ppm.pack(px.tobytes(), w, depth, colour, None, 256)
        assert st == 0
        packed.append(np.frombuffer(pix, dtype=np.uint8))
        records.append(mm.words(mm.record(w, h, depth, colour)))
    records.insert(1, mm.words(mm.record(4, 4, 0, 0)))          # a dimension record among the good ones: not this call's to take
    packed.insert(1, np.zeros(16, dtype=np.uint8))
    pix, p_off = gh.dev(np.concatenate(packed)), gh.dev(gh.offsets([p.size for p in packed]))
    info = gh.dev(np.array(records, dtype=np.uint32).view(np.int32))
    file, f_off, f_len, st, _ = pcs.png_encode_mixed_files_level_pieces_batch(pix, p_off, info, level, piece_bytes=piece_bytes)
    torch.cuda.synchronize()
    want_st = [0] * len(ks)
    want_st.insert(1, 3)
    assert st.cpu().tolist() == want_st
    want = [expected[k][1] if piece_bytes == 65536 or level == 0 else _in_pieces(expected[k][1], level, piece_bytes) for k in ks]
    want.insert(1, b"")
    assert _files(file, f_off, f_len) == want


def test_callers_file_slots_in_pieces():
    """The default slots are the bound's; in the caller's slots a file that does not fit is status 2 with file_len 0, and
    the others are written between their guards; the slots of the pictures that fail upstream stay untouched."""
    import torch
    import fdeflate_amd.pieces as pcs
    import png_file_model as fm
    level, piece_bytes = 6, 1000
    cases, expected = lc.cases8(), lc.expected8(level)
    rgba, r_off, width, height, pairs = _collection(cases)
    _, d_off, _, _, _ = pcs.png_encode_mixed_rgba_files_level_pieces_batch(rgba, r_off, width, height, level, pairs=pairs, piece_bytes=piece_bytes)
    torch.cuda.synchronize()
    bound = np.diff(d_off.cpu().numpy())
    files = [_in_pieces(e[1], level, piece_bytes) if e[0] == 0 else None for e in expected]
    for k, (st, f, depth, colour) in enumerate(expected):
        if st == 0:
            rb = fm.geometry(cases[k][2], depth, colour)[0]
            assert bound[k] == pcs.pieces_file_bound(cases[k][3], rb, level, piece_bytes, f.index(b"IDAT") + 4) >= len(files[k]), cases[k][0]
    good = [k for k, e in enumerate(expected) if e[0] == 0]
    tight = good[0]         # the tiled picture: six pieces
    sizes = np.array([len(f) + 2 if f else 0 for f in files], dtype=np.int64)
    sizes[tight] = len(files[tight]) - 1
    own_off = gh.offsets(sizes, 7)
    own = torch.full((int(own_off[-1]) + 11,), GUARD, dtype=torch.uint8, device="cuda")
    _, _, own_len, own_st, _ = pcs.png_encode_mixed_rgba_files_level_pieces_batch(rgba, r_off, width, height, level, pairs=pairs, file=own,
                                                                                 file_off=gh.dev(own_off), piece_bytes=piece_bytes)
    torch.cuda.synchronize()
    # (a picture the plan accepts and the packer would refuse: its empty slot is found first, 2 in front of 13)
    assert own_st.cpu().tolist() == [2 if k == tight or e[0] == 13 else e[0] for k, e in enumerate(expected)]
    want = np.full(own.numel(), GUARD, dtype=np.uint8)
    for k, f in enumerate(files):
        if f and k != tight:
            want[own_off[k]:own_off[k] + len(f)] = np.frombuffer(f, dtype=np.uint8)
    assert own_len.cpu().tolist() == [len(f) if f and k != tight else 0 for k, f in enumerate(files)]
    host = own.cpu().numpy()
    # (as in the whole-stream pipelines, the framing finds the file a byte too long behind the encoder: the slot holds stream bytes)
    want[own_off[tight]:own_off[tight + 1]] = host[own_off[tight]:own_off[tight + 1]]
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, "first differing byte at %d" % bad[0]
