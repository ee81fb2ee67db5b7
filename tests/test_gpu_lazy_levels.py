"""-m gpu: encoder levels 4-9 (LazyParser + HybridMatchFinder, include/fdeflate_hip_levels.h) on the GPU against
tests/lazy_model.py, bit-exact, in the shapes of tests/test_gpu_levels.py.  The model's shared pieces are pinned against
the oracle at level 1 and RLE (tests/test_level_model.py); the hybrid finder and the lazy loop are stated twice, in the
model and in the oracle's C, and tests/test_oracle_levels.py holds the two to the same bytes and branch counts (the real
crate cannot be run here).  The inputs and the model's results (lazy_model.model_results, once per process) are the ones
tests/test_lazy_model.py checks on the CPU; tests/test_gpu_levels_oracle.py compares the same kernels with the oracle
on 2 000 streams per level."""
import ctypes as C

import numpy as np
import pytest

import lazy_model as zm
import level_model as lm
import oracle_binding as ob
import streams

pytestmark = pytest.mark.gpu

EMPTY = bytes.fromhex("7801030000000001")
LEVELS = (4, 5, 6, 9)


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


def _ragged():
    r = np.random.default_rng(17)
    raws = []
    for _ in range(70):   # more than one wavefront of streams, ragged sizes
        n = int(r.integers(0, 9000))
        raws.append(bytes(r.integers(0, int(r.integers(2, 256)), n, dtype=np.uint8)))
    return raws


@pytest.fixture(scope="module")
def cases():
    """level -> (inputs, expected streams): lazy_model.shared_inputs() and 70 ragged random streams of 0 .. 9 000 bytes."""
    ragged = _ragged()
    res = {}
    for level in LEVELS:
        rows = zm.model_results()[level]
        res[level] = ([x for x, _, _ in rows] + ragged, [o for _, o, _ in rows] + [zm.compress(x, level) for x in ragged])
    return res


def _encode(level):
    from fdeflate_amd import levels
    return lambda a, b, c, d: levels.deflate_level_batch(a, b, c, d, level)


@pytest.mark.parametrize("launch", [None, "lanes=1", "lanes=64", "resident=64"])
@pytest.mark.parametrize("level", LEVELS)
def test_lazy_levels_bit_exact(harness, cases, level, launch, monkeypatch):
    """fdh_deflate_level_batch, one batch per level, guard bytes 0x5A behind every stream: the library's own launch shape,
    1 and 64 streams per wavefront (FDH_GEN_LANES), and more streams than are resident at once (FDH_GEN_RESIDENT=64 with
    16 lanes: every wavefront takes further rounds, so tables are reused by a later stream -- the head table and the
    4-table cleared again, the link ring not)."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import levels
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    if launch is not None:
        k, v = launch.split("=")
        monkeypatch.setenv({"lanes": "FDH_GEN_LANES", "resident": "FDH_GEN_RESIDENT"}[k], v)
        if k == "resident":
            monkeypatch.setenv("FDH_GEN_LANES", "16")
    raws, expect = cases[level]
    buf, in_off = streams.pack_exact(raws)
    caps = [fd.compress_bound(len(x)) + 5 for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
    ln = levels.deflate_level_batch(torch.from_numpy(buf).cuda(), torch.from_numpy(in_off.astype(np.int64)).cuda(), d_out,
                                    torch.from_numpy(out_off).cuda(), level).cpu().numpy().view(np.uint32)
    h = d_out.cpu().numpy()
    for i, raw in enumerate(raws):
        got = h[out_off[i]:out_off[i] + int(ln[i])].tobytes()
        assert got == expect[i], (launch, level, i, len(raw), int(ln[i]), len(expect[i]))
        assert np.all(h[out_off[i] + int(ln[i]):out_off[i + 1]] == 0x5A), (launch, level, i)


def test_levels_0_to_3_through_the_new_call_equal_the_existing_calls(harness, monkeypatch):
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import levels
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    raws = streams.encoder_inputs()[:18] + _ragged()[:20]
    buf, in_off = streams.pack_exact(raws)
    caps = [max(fd.compress_bound(len(x)), fd.stored_size(len(x))) for x in raws]
    out_off = np.zeros(len(raws) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_in, d_in_off, d_out_off = torch.from_numpy(buf).cuda(), torch.from_numpy(in_off.astype(np.int64)).cuda(), torch.from_numpy(out_off).cuda()
    old = {0: lambda o: fd.deflate_stored_batch(d_in, d_in_off, o, d_out_off),
           1: lambda o: fd.deflate_general_batch(d_in, d_in_off, o, d_out_off, fd.MODE_LEVEL1),
           2: lambda o: fd.deflate_general_batch(d_in, d_in_off, o, d_out_off, fd.MODE_LEVEL2),
           3: lambda o: fd.deflate_general_batch(d_in, d_in_off, o, d_out_off, fd.MODE_LEVEL3)}
    for level in (0, 1, 2, 3):
        a = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        b = a.clone()
        la = old[level](a)
        lb = levels.deflate_level_batch(d_in, d_in_off, b, d_out_off, level)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a, b), level
        assert int(la.min()) > 0


def test_levels_7_8_and_9_are_identical(harness, cases, monkeypatch):
    """Levels 7 and 8 against level 9's model output, and over the volume corpus (tests/level_volume.py) against bytes the
    oracle computed AT 7 and AT 8, so that the two levels are not pinned by their equality with 9 alone."""
    import fdeflate_amd as fd
    import level_volume
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    for level in (7, 8):
        level_volume.gpu_compare_with_oracle(level, None, "levels 7 and 8")
    raws, want = cases[9]
    raws, want = raws[-90:], want[-90:]     # the lazy inputs and the ragged streams
    caps = [fd.compress_bound(len(x)) for x in raws]
    for level in (7, 8):
        ln, slots, faults = harness.gpu_encode_slots(_encode(level), raws, caps, EMPTY)
        assert not faults, (level, faults[:8])
        for i, w in enumerate(want):
            assert int(ln[i]) == len(w) and slots[i][:len(w)].tobytes() == w, (level, i, len(raws[i]), int(ln[i]), len(w))


@pytest.mark.parametrize("lanes", [None, "1", "64"])
@pytest.mark.parametrize("level", LEVELS)
def test_lazy_levels_slots_too_small(harness, cases, level, lanes, monkeypatch):
    """Every third slot too small (by one byte, by half, 1 byte, 0 bytes long in turn), the others exactly the compressed
    length or the bound, at odd alignments with guard slots between: out_len = 0xFFFFFFFF for exactly the small ones, no
    byte outside any slot changed, every other stream bit-exact."""
    import fdeflate_amd as fd
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    if lanes is None:
        monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    else:
        monkeypatch.setenv("FDH_GEN_LANES", lanes)
    raws, want = cases[level]
    caps, small = [], []
    for i, w in enumerate(want):
        if i % 3 == 1:
            caps.append((len(w) - 1, len(w) // 2, 1, 0)[(i // 3) % 4])
            small.append(True)
        else:
            caps.append(len(w) if i % 3 == 0 else fd.compress_bound(len(raws[i])))
            small.append(False)
    ln, slots, faults = harness.gpu_encode_slots(_encode(level), raws, caps, EMPTY)
    assert not faults, (level, lanes, faults[:8])
    for i, w in enumerate(want):
        if small[i]:
            assert int(ln[i]) == 0xFFFFFFFF, (level, lanes, i, len(w), slots[i].size, int(ln[i]))
            continue
        assert int(ln[i]) == len(w), (level, lanes, i, int(ln[i]), len(w))
        assert slots[i][:len(w)].tobytes() == w, (level, lanes, i, "not bit-exact next to an overflowing neighbour")
        assert np.all(slots[i][len(w):] == 0x5A), (level, lanes, i, "wrote behind its stream")


def _c_compress_level(data, level):
    from fdeflate_amd import _lib
    L = _lib.lib()
    out, n = C.c_void_p(), C.c_size_t()
    rc = L.fdh_compress_to_vec_level(data, len(data), level, C.byref(out), C.byref(n))
    if rc != 0:
        return rc, None
    try:
        return 0, C.string_at(out.value, n.value)
    finally:
        L.fdh_free(out)


def test_host_one_shot_at_every_level(harness):
    """fdh_compress_to_vec_level and levels.compress_to_vec_with_level: level 0 stored, 1 the oracle's level 1, 2 and 3
    level_model, 4-9 lazy_model; the empty input; level 10 and above refused with a message."""
    import fdeflate_amd as fd
    from fdeflate_amd import _lib, levels
    r = np.random.default_rng(31)
    datas = [b"", b"x", b"Hello world! " * 100, bytes(r.integers(0, 4, 40000, dtype=np.uint8))]
    for data in datas:
        want = {0: ob.compress_stored(data), 1: ob.compress_level1(data), 2: lm.compress(data, 2), 3: lm.compress(data, 3)}
        for level in (4, 5, 6, 7):
            want[level] = zm.compress(data, level)
        want[8] = want[9] = want[7]
        for level in range(10):
            rc, got = _c_compress_level(data, level)
            assert rc == 0 and got == want[level], (len(data), level)
            assert levels.compress_to_vec_with_level(data, level) == want[level], (len(data), level)
        assert fd.decompress_to_vec(want[6]) == data and fd.decompress_to_vec(want[9]) == data
    for level in range(1, 10):
        assert _c_compress_level(b"", level) == (0, EMPTY)
    for level in (10, 255, 0xFFFFFFFF):
        rc, got = _c_compress_level(b"abc", level)
        assert rc == 1 and got is None, level     # FDH_ERR_INVALID_ARGUMENT
        msg = _lib.lib().fdh_last_error().decode()
        assert msg and "level" in msg, msg
    with pytest.raises(ValueError):
        levels.compress_to_vec_with_level(b"abc", 10)


def test_level_10_is_refused_by_the_batch_call(harness):
    import torch
    from fdeflate_amd import _lib, levels
    d_in = torch.zeros(16, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 16], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    o_off = torch.tensor([0, 2048], dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        levels.deflate_level_batch(d_in, off, d_out, o_off, 10)
    ln = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().fdh_deflate_level_batch(d_in.data_ptr(), off.data_ptr(), d_out.data_ptr(), o_off.data_ptr(), ln.data_ptr(), 1, 10, None)
    assert rc == 1 and "level" in _lib.lib().fdh_last_error().decode()


def test_level_6_roundtrip_at_moderate_scale(harness):
    """1 024 x 64 KiB through level 6 on the GPU, decoded again on the GPU: every stream Ok, lengths exact, decoded == raw,
    reported Adler-32 == the trailer the encoder wrote; the model byte-compares 8 strided streams, the oracle's C
    restatement of level 6 all 1 024 (k = 1: 64 MiB on 16 threads took it 0.1 s on the GPU machine's host; 0.4 s
    extrapolated from 256 streams on the 8 cores of the build machine; the run prints its own time)."""
    import torch
    import fdeflate_amd as fd
    import level_volume
    from fdeflate_amd import levels, synth
    n, L = 1024, 65536
    raw = synth.gen_batch_torch(40000, n, L)
    bound = (fd.compress_bound(L) + 15) & ~15
    in_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
    c_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * bound
    comp = torch.zeros(n * bound, dtype=torch.uint8, device="cuda")
    clen = levels.deflate_level_batch(raw.view(-1), in_off, comp, c_off, 6)
    clen_h = clen.cpu().numpy().view(np.uint32)
    assert int(clen_h.max()) <= bound
    print("level 6: %d x %d bytes -> %d compressed bytes" % (n, L, int(clen_h.astype(np.int64).sum())))
    for i in range(0, n, 128):
        exp = zm.compress(raw[i].cpu().numpy().tobytes(), 6)
        got = comp[i * bound:i * bound + int(clen_h[i])].cpu().numpy().tobytes()
        assert got == exp, i
    bad, dt = level_volume.mismatches_against_oracle(raw, comp, clen, bound, 6)
    print("oracle, level 6, %d streams: %.1f s" % (n, dt))
    assert not bad, (len(bad), bad[:8])
    out = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    out_len, status, adler = fd.inflate_batch(comp, c_off, out, in_off)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and bool((out_len == L).all()) and torch.equal(out, raw.view(-1))
    idx = (c_off[:-1] + clen.to(torch.int64))[:, None] + torch.arange(-4, 0, device="cuda")[None, :]
    tr = comp[idx].to(torch.int64)
    trailer = (tr[:, 0] << 24) | (tr[:, 1] << 16) | (tr[:, 2] << 8) | tr[:, 3]
    assert torch.equal(trailer, adler.to(torch.int64) & 0xFFFFFFFF)
