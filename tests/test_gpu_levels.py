"""-m gpu: encoder levels 2 and 3 (GreedyParser + HashChainMatchFinder) on the GPU against
tests/level_model.py, bit-exact.  The model is pinned against the oracle at level 1 and RLE by tests/test_level_model.py
and at levels 2 and 3, where both state the chain finder, by tests/test_oracle_levels.py; the input set (tests/streams.py) and the model's results
(level_model.model_results, computed once per process) are the ones that file checks."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import level_model as lm
import oracle_binding as ob
import streams

pytestmark = pytest.mark.gpu

EMPTY = bytes.fromhex("7801030000000001")


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


def _modes():
    import fdeflate_amd as fd
    return ((2, fd.MODE_LEVEL2), (3, fd.MODE_LEVEL3))


def _ragged():
    r = np.random.default_rng(17)
    raws = []
    for _ in range(70):   # more than one wavefront of streams, ragged sizes
        n = int(r.integers(0, 9000))
        raws.append(bytes(r.integers(0, int(r.integers(2, 256)), n, dtype=np.uint8)))
    return raws


@pytest.fixture(scope="module")
def cases():
    """level -> (inputs, expected streams): the encoder inputs, the chain inputs and 70 ragged random streams."""
    ragged = _ragged()
    res = {}
    for level in (2, 3):
        rows = lm.model_results()[level]
        res[level] = ([x for x, _, _ in rows] + ragged, [o for _, o, _ in rows] + [lm.compress(x, level) for x in ragged])
    return res


@pytest.mark.parametrize("launch", [None, "lanes=1", "lanes=64", "resident=64"])
def test_levels_2_and_3_bit_exact(harness, cases, launch, monkeypatch):
    """fdh_deflate_general_batch with FDH_MODE_LEVEL2 / FDH_MODE_LEVEL3, one batch, guard bytes 0x5A behind every
    stream: the library's own launch shape, 1 and 64 streams per wavefront (FDH_GEN_LANES), and more streams than
    are resident at once (FDH_GEN_RESIDENT=64: every wavefront takes a second round, so tables are reused by a
    later stream -- the head tables cleared again, the link rings not)."""
    import torch
    import fdeflate_amd as fd
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    if launch is not None:
        k, v = launch.split("=")
        monkeypatch.setenv({"lanes": "FDH_GEN_LANES", "resident": "FDH_GEN_RESIDENT"}[k], v)
        if k == "resident":
            monkeypatch.setenv("FDH_GEN_LANES", "16")
    for level, mode in _modes():
        raws, expect = cases[level]
        buf, in_off = streams.pack_exact(raws)
        caps = [fd.compress_bound(len(x)) + 5 for x in raws]
        out_off = np.zeros(len(raws) + 1, dtype=np.int64)
        out_off[1:] = np.cumsum(caps)
        d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        ln = fd.deflate_general_batch(torch.from_numpy(buf).cuda(), torch.from_numpy(in_off.astype(np.int64)).cuda(), d_out,
                                      torch.from_numpy(out_off).cuda(), mode).cpu().numpy().view(np.uint32)
        h = d_out.cpu().numpy()
        for i, raw in enumerate(raws):
            got = h[out_off[i]:out_off[i] + int(ln[i])].tobytes()
            assert got == expect[i], (launch, level, i, len(raw), int(ln[i]), len(expect[i]))
            assert np.all(h[out_off[i] + int(ln[i]):out_off[i + 1]] == 0x5A), (launch, level, i)


def _c_compress_with_level(data, level, symbol="fdh_compress_to_vec_with_level"):
    from fdeflate_amd import _lib
    L = _lib.lib()
    out, n = C.c_void_p(), C.c_size_t()
    rc = getattr(L, symbol)(data, len(data), level, C.byref(out), C.byref(n))
    if rc != 0:
        return rc, None
    try:
        return 0, C.string_at(out.value, n.value)
    finally:
        L.fdh_free(out)


def test_compress_to_vec_with_level_host_entry_points(harness):
    """fdh_compress_to_vec_with_level and fd.compress_to_vec_with_level: level 0 stored, level 1 the oracle's level 1,
    levels 2 and 3 the model; level 4 and above FDH_ERR_INVALID_ARGUMENT with a message; the empty input."""
    import fdeflate_amd as fd
    from fdeflate_amd import _lib
    r = np.random.default_rng(31)
    datas = [b"", b"x", b"Hello world! " * 100, bytes(r.integers(0, 4, 40000, dtype=np.uint8))]
    for data in datas:
        want = {0: ob.compress_stored(data), 1: ob.compress_level1(data), 2: lm.compress(data, 2), 3: lm.compress(data, 3)}
        for level in (0, 1, 2, 3):
            rc, got = _c_compress_with_level(data, level)
            assert rc == 0 and got == want[level], (len(data), level)
            assert fd.compress_to_vec_with_level(data, level) == want[level], (len(data), level)
        assert fd.decompress_to_vec(want[3]) == data
    for level in (1, 2, 3):
        assert _c_compress_with_level(b"", level) == (0, EMPTY)
    for level in (4, 9, 10, 0xFFFFFFFF):
        rc, got = _c_compress_with_level(b"abc", level)
        assert rc == 1 and got is None, level     # FDH_ERR_INVALID_ARGUMENT
        msg = _lib.lib().fdh_last_error().decode()
        assert msg and "level" in msg, msg
    with pytest.raises(ValueError):
        fd.compress_to_vec_with_level(b"abc", 4)


def test_unknown_modes_are_still_refused(harness):
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd._lib import FdeflateHipError
    d_in = torch.zeros(16, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 16], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    o_off = torch.tensor([0, 2048], dtype=torch.int64, device="cuda")
    for mode in (0, 5, 99):
        with pytest.raises(FdeflateHipError):
            fd.deflate_general_batch(d_in, off, d_out, o_off, mode)


@pytest.mark.parametrize("level", range(10))
def test_every_door_to_a_level_gives_the_same_bytes(harness, level, monkeypatch):
    """Inputs of 0, 1, 300 and 70 000 bytes (the last longer than the 32 KiB window), one batch per door, the streams
    compared whole: fdh_deflate_level_batch, fdh_compress_to_vec_level and deflate_level_pieces_batch with one piece per
    input at every level; at levels 0 .. 3 also fdh_compress_to_vec_with_level and the batch call that level had before
    (fdh_deflate_stored_batch, fdh_deflate_general_batch in the level's mode)."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import levels, pieces
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    raws = [streams._vol_text(streams.rng(5 + n), n) for n in (0, 1, 300, 70000)]
    assert [len(x) for x in raws] == [0, 1, 300, 70000]
    one_piece = 1 << 17
    buf, in_off = streams.pack_exact(raws)
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum([max(fd.stored_size(len(x)), pieces.pieces_bound(len(x), level, one_piece)) for x in raws])
    d_in, d_in_off, d_out_off = torch.from_numpy(buf).cuda(), torch.from_numpy(in_off.astype(np.int64)).cuda(), torch.from_numpy(out_off).cuda()

    def batch(door):
        out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        ln = door(d_in, d_in_off, out, d_out_off).cpu().numpy().view(np.uint32)
        h = out.cpu().numpy()
        return [h[out_off[i]:out_off[i] + int(ln[i])].tobytes() for i in range(len(raws))]

    doors = {"level_batch": batch(lambda a, b, c, d: levels.deflate_level_batch(a, b, c, d, level)),
             "one piece each": batch(lambda a, b, c, d: pieces.deflate_level_pieces_batch(a, b, c, d, level, one_piece)),
             "to_vec_level": [_c_compress_with_level(x, level, "fdh_compress_to_vec_level")[1] for x in raws]}
    if level <= 3:
        modes = (None, fd.MODE_LEVEL1, fd.MODE_LEVEL2, fd.MODE_LEVEL3)
        doors["to_vec_with_level"] = [_c_compress_with_level(x, level)[1] for x in raws]
        doors["the level's own batch call"] = batch(fd.deflate_stored_batch if level == 0 else
                                                    lambda a, b, c, d: fd.deflate_general_batch(a, b, c, d, modes[level]))
    want = doors["level_batch"]
    assert all(len(w) >= 8 for w in want) and (level == 0 or want[0] == EMPTY)
    assert level == 0 or len(want[3]) < 35000           # compressed: the doors do not agree on a stored stream
    for name, got in doors.items():
        assert got == want, (level, name, [None if g is None else len(g) for g in got], [len(w) for w in want])


@pytest.mark.parametrize("lanes", [None, "1", "64"])
def test_levels_2_and_3_slots_too_small(harness, cases, lanes, monkeypatch):
    """Every third slot too small (by one byte, by half, 1 byte, 0 bytes long in turn), the others exactly the
    compressed length or the bound, at odd alignments with guard slots between: out_len = 0xFFFFFFFF for exactly the
    small ones, no byte outside any slot changed, every other stream bit-exact.  The set holds the 300 000-byte inputs,
    whose first pass writes more than 32 KiB, so that the second pass starts past 0."""
    import fdeflate_amd as fd
    if lanes is None:
        monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    else:
        monkeypatch.setenv("FDH_GEN_LANES", lanes)
    for level, mode in _modes():
        raws, want = cases[level]
        caps, small = [], []
        for i, w in enumerate(want):
            if i % 3 == 1:
                caps.append((len(w) - 1, len(w) // 2, 1, 0)[(i // 3) % 4])
                small.append(True)
            else:
                caps.append(len(w) if i % 3 == 0 else fd.compress_bound(len(raws[i])))
                small.append(False)
        assert any(small[i] and len(raws[i]) == 300000 for i in range(len(raws))) and \
            any(not small[i] and len(raws[i]) == 300000 for i in range(len(raws)))
        ln, slots, faults = harness.gpu_encode_slots(
            lambda a, b, c, d: fd.deflate_general_batch(a, b, c, d, mode), raws, caps, EMPTY)
        assert not faults, (level, lanes, faults[:8])
        for i, w in enumerate(want):
            if small[i]:
                assert int(ln[i]) == 0xFFFFFFFF, (level, lanes, i, len(w), slots[i].size, int(ln[i]))
                continue
            assert int(ln[i]) == len(w), (level, lanes, i, int(ln[i]), len(w))
            assert slots[i][:len(w)].tobytes() == w, (level, lanes, i, "not bit-exact next to an overflowing neighbour")
            assert np.all(slots[i][len(w):] == 0x5A), (level, lanes, i, "wrote behind its stream")


def test_levels_2_and_3_one_block_over_2_22_positions(harness):
    """4.5 MiB of bytes without repeats is ONE block (a literal run counts as one symbol): the block writer's 64-bit
    heap items; bit-exact with the model at both levels, next to a short stream, and in a slot one byte too small."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(23)
    big = r.integers(0, 256, 4_718_592 + 11, dtype=np.uint8).tobytes()
    raws = [big, b"abcabcabcabc" * 50, big]
    for level, mode in _modes():
        t0 = time.time()
        exp_big = lm.compress(big, level)
        want = [exp_big, lm.compress(raws[1], level), exp_big]
        print("model, level %d, %d bytes: %.1f s" % (level, len(big), time.time() - t0))
        caps = [fd.compress_bound(len(big)), fd.compress_bound(len(raws[1])), len(exp_big) - 1]
        ln, slots, faults = harness.gpu_encode_slots(
            lambda a, b, c, d: fd.deflate_general_batch(a, b, c, d, mode), raws, caps, EMPTY)
        assert not faults, (level, faults[:8])
        for i in (0, 1):
            assert int(ln[i]) == len(want[i]) and slots[i][:len(want[i])].tobytes() == want[i], (level, i, int(ln[i]), len(want[i]))
        assert int(ln[2]) == 0xFFFFFFFF, (level, int(ln[2]))


def test_levels_2_and_3_roundtrip_at_scale(harness):
    """8192 x 64 KiB through levels 2 and 3 on the GPU, decoded again on the GPU: every stream Ok, lengths exact,
    decoded == raw, reported Adler-32 == the trailer the encoder wrote; the model byte-compares a strided sample of
    64 compressed streams (4 MiB of input per level: the model is Python), and the oracle's C restatement of the levels
    every one of the 8 192 (k = 1: 512 MiB on 16 threads took it 0.1 s at level 2 and 0.2 s at level 3 on the GPU machine's
    host, against 0.7 s and 2.9 s for the model's 64; 0.6 s and 1.3 s extrapolated from 256 streams on the 8 cores of the
    build machine; the run prints its own time)."""
    import torch
    import fdeflate_amd as fd
    import level_volume
    from fdeflate_amd import synth
    n, L = 8192, 65536
    raw = synth.gen_batch_torch(40000, n, L)
    bound = (fd.compress_bound(L) + 15) & ~15
    in_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    c_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * bound
    for level, mode in _modes():
        comp = torch.zeros(n * bound, dtype=torch.uint8, device="cuda")
        clen = fd.deflate_general_batch(raw.view(-1), in_off, comp, c_off, mode)
        clen_h = clen.cpu().numpy().view(np.uint32)
        assert int(clen_h.max()) <= bound
        print("level %d: %d x %d bytes -> %d compressed bytes" % (level, n, L, int(clen_h.astype(np.int64).sum())))
        t0 = time.time()
        for i in range(0, n, 128):
            exp = lm.compress(raw[i].cpu().numpy().tobytes(), level)
            got = comp[i * bound:i * bound + int(clen_h[i])].cpu().numpy().tobytes()
            assert got == exp, (level, i)
        print("model, level %d, 64 streams: %.1f s" % (level, time.time() - t0))
        bad, dt = level_volume.mismatches_against_oracle(raw, comp, clen, bound, level)
        print("oracle, level %d, %d streams: %.1f s" % (level, n, dt))
        assert not bad, (level, len(bad), bad[:8])
        out = torch.empty(n * L, dtype=torch.uint8, device="cuda")
        out_len, status, adler = fd.inflate_batch(comp, c_off, out, in_off)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0 and bool((out_len == L).all()) and torch.equal(out, raw.view(-1)), level
        idx = (c_off[:-1] + clen.to(torch.int64))[:, None] + torch.arange(-4, 0, device="cuda")[None, :]
        tr = comp[idx].to(torch.int64)
        trailer = (tr[:, 0] << 24) | (tr[:, 1] << 16) | (tr[:, 2] << 8) | tr[:, 3]
        assert torch.equal(trailer, adler.to(torch.int64) & 0xFFFFFFFF), level
        del comp, out


@pytest.fixture(scope="module")
def edge_cases():
    """(inputs, mode -> expected streams) over streams.run_edge_inputs(), which ends with the late-match family: the
    oracle's bytes at level 1 and RLE, the model's at levels 2 and 3 (the tail of level_model.model_results())."""
    import fdeflate_amd as fd
    raws = streams.run_edge_inputs()
    want = {fd.MODE_LEVEL1: [ob.compress_level1(x) for x in raws], fd.MODE_RLE: [ob.compress_rle(x) for x in raws]}
    for level, mode in _modes():
        rows = lm.model_results()[level][-len(raws):]
        assert [x for x, _, _ in rows] == raws
        want[mode] = [o for _, o, _ in rows]
    return raws, want


@pytest.mark.parametrize("lanes", [None, "1"])
def test_run_edge_inputs_bit_exact_in_all_four_modes(harness, edge_cases, lanes, monkeypatch):
    """The inputs that take the parser's counter of equal bytes through every exit (tests/test_level_model.py counts
    them), one batch per mode with guard bytes behind every slot: bit-exact at the library's own launch shape and with
    one stream per wavefront."""
    import fdeflate_amd as fd
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    if lanes is None:
        monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    else:
        monkeypatch.setenv("FDH_GEN_LANES", lanes)
    raws, want = edge_cases
    caps = [fd.compress_bound(len(x)) for x in raws]
    for mode in (fd.MODE_LEVEL1, fd.MODE_RLE, fd.MODE_LEVEL2, fd.MODE_LEVEL3):
        ln, slots, faults = harness.gpu_encode_slots(
            lambda a, b, c, d: fd.deflate_general_batch(a, b, c, d, mode), raws, caps, EMPTY)
        assert not faults, (mode, lanes, faults[:8])
        for i, w in enumerate(want[mode]):
            assert int(ln[i]) == len(w) and slots[i][:len(w)].tobytes() == w, (mode, lanes, i, len(raws[i]), int(ln[i]), len(w))
            assert np.all(slots[i][len(w):] == 0x5A), (mode, lanes, i, "wrote behind its stream")
