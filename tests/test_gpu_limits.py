"""-m gpu: parity at every SIZE gate of the decode chain and of the encoders (DESIGN.md "Size gates").

The kernels of fdh_inflate_batch hand a stream on when it is "not theirs"; several of those decisions are pure size
gates (compressed length, slot length).  Every test here puts streams just under, exactly at and just over one gate and
decodes them (a) with the whole pipeline, which must be bit-exact -- status, length, bytes, Adler-32 -- and (b) with the
kernel in question alone, which must leave the stream at / over its gate PENDING with slot and guards untouched and be
right about whatever it reports.  The encoders get slots that are too small and inputs that are too long.

The reference of a VALID stream is the raw buffer it was made from, zlib.adler32 of it and status Ok (zlib.decompress of
the blob gives the same bytes: the oracle's encoder is not part of the expectation); the oracle decides short slots,
cuts and damaged copies, where it alone knows status and partial length.  A blob is brought to an exact length by junk
behind its Adler-32 trailer, which every decoder ignores (src/decompress.rs:185-187) -- the oracle decodes each padded
blob once to pin that.  Big slots never come back to the host (gpu_harness.gpu_inflate_big)."""
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_binding as ob
import streams

pytestmark = pytest.mark.gpu

PENDING = 0xFFFFFFFF
PENDING_ANY = 0xFFFFFFFD        # the LZ-window kernel also leaves PENDING_SERIAL / PENDING_RESUME
LANDING_ONLY = 0x20000          # FDH_FLAG_LANDING_ONLY
INTERVAL_ONLY = 0x800 | 0x10000  # FDH_FLAG_INTERVALS_ONLY without the landing decoder in front of it (NO_LANDING)
LANDING_INTERVAL = 0x800        # ... with it: both kernels share the gates
SEGMENT_ONLY = 0x400 | 64       # NO_INTERVALS | FIRST_ONLY: the segment kernel is the first and only one
LANES_ONLY = 128 | 16 | 64      # NO_SEGMENTS | FORCE_LANES | FIRST_ONLY: the stream-per-lane kernel alone
LZ_ONLY = 0x2000                # nothing behind the LZ-window kernel runs
NO_CHECKPOINTS = 0x4000


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


def _need(nbytes, what):
    """Skips only when the device does not have the memory free (never on an MI355X that is not full)."""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB free of %.1f" % (what, nbytes / 2**30, free / 2**30, total / 2**30))


def _bench(sid, n):
    """The bench's buffers: sid % 16 == 7 has every other row zero, 15 is all zero, the others are noisy rows."""
    from fdeflate_amd import synth
    return synth.gen_stream_np(sid, n).tobytes()


def _scaled_to(make_raw, encode, target, probe_len, tol):
    """A (raw, blob) whose blob is target - tol .. target bytes long: the length of the raw buffer is scaled from one
    probe encode (the content is homogeneous), and checked."""
    c0 = len(encode(make_raw(probe_len)))
    n = int(probe_len * (target - tol // 2) / c0)
    raw = make_raw(n)
    blob = encode(raw)
    assert target - tol <= len(blob) <= target, (len(blob), target, n)
    return raw, blob


def _inflate_py(blob):
    return zlib.decompressobj().decompress(bytes(blob))


def _oracle_decodes(blob, raw):
    st, out, ad = ob.decompress_bounded(blob, len(raw))
    return st == 0 and out == bytes(raw) and ad == zlib.adler32(raw)


def _oracle_pins_padding(blob, raw):
    assert _oracle_decodes(blob, raw), "junk behind the trailer changed the oracle's answer"


def _assert_whole(h, names, blobs, caps, raws, flags=0):
    """Whole pipeline on valid streams in slots that hold them: Ok, the raw buffer's length, bytes and Adler-32; nothing
    behind the bytes, nothing in the guards."""
    st, ln, ad, slots, guards_ok = h.gpu_inflate_big(blobs, caps, flags=flags)
    assert guards_ok, ("a kernel wrote outside its output slot", hex(flags))
    bad = []
    for i, name in enumerate(names):
        raw = raws[i]
        if int(st[i]) != 0:
            bad.append((name, "status", hex(int(st[i]))))
        elif int(ln[i]) != len(raw):
            bad.append((name, "len", int(ln[i]), len(raw)))
        elif int(ad[i]) != zlib.adler32(raw):
            bad.append((name, "adler", hex(int(ad[i])), hex(zlib.adler32(raw))))
        elif not slots.head_equals(i, raw):
            bad.append((name, "bytes"))
        elif not slots.untouched(i, len(raw)):
            bad.append((name, "wrote behind its output"))
    assert not bad, (hex(flags), bad[:10])


def _assert_alone(h, names, blobs, caps, raws, flags, take=(), leave=(), pend_min=PENDING, one_by_one=False):
    """One kernel alone on valid streams: what it reports is Ok and right; the streams of `leave` (at / over its gate)
    come back PENDING with the slot untouched; the streams of `take` are finished by it."""
    groups = [[i] for i in range(len(names))] if one_by_one else [list(range(len(names)))]
    for g in groups:
        st, ln, ad, slots, guards_ok = h.gpu_inflate_big([blobs[i] for i in g], [caps[i] for i in g], flags=flags)
        assert guards_ok, ("a kernel wrote outside its output slot", hex(flags))
        for k, i in enumerate(g):
            name, raw = names[i], raws[i]
            if int(st[k]) >= pend_min:
                assert name not in take, (name, "left PENDING by the kernel that should take it", hex(flags))
                if name in leave:
                    assert slots.untouched(k), (name, "PENDING, but its slot was written", hex(flags))
                continue
            assert name not in leave, (name, "taken on the wrong side of the gate", hex(flags), hex(int(st[k])))
            assert int(st[k]) == 0, (name, hex(int(st[k])), hex(flags))
            assert int(ln[k]) == len(raw) and int(ad[k]) == zlib.adler32(raw), (name, hex(flags))
            assert slots.head_equals(k, raw) and slots.untouched(k, len(raw)), (name, hex(flags))


def _assert_oracle(h, names, blobs, caps, flags=0):
    """Short slots, cuts, damaged copies: the oracle's status; length and bytes whenever the reference defines them (Ok,
    OutputTooLarge, and the partial output of InsufficientInput: include/fdeflate_hip.h), Adler-32 for Ok.  What lies
    in the slot behind the reported length of a result that is not Ok is not checked: the header promises the bytes up
    to out_len and that nothing outside the slot is written, and a kernel that handed a damaged stream on may have
    written further into the slot than the exact decoder then reports (for Ok, _assert_whole checks the rest)."""
    st, ln, ad, slots, guards_ok = h.gpu_inflate_big(blobs, caps, flags=flags)
    assert guards_ok, ("a kernel wrote outside its output slot", hex(flags))
    bad = []
    for i, name in enumerate(names):
        rs, out, ra = ob.decompress_bounded(blobs[i], caps[i], bool(flags & 1))
        if int(st[i]) != rs:
            bad.append((name, "status", hex(int(st[i])), ob.STATUS_NAMES[rs]))
        elif rs in (0, 2, 17):
            if int(ln[i]) != len(out):
                bad.append((name, "len", int(ln[i]), len(out), ob.STATUS_NAMES[rs]))
            elif not slots.head_equals(i, out):
                bad.append((name, "bytes", ob.STATUS_NAMES[rs]))
            elif rs == 0 and int(ad[i]) != ra:
                bad.append((name, "adler"))
    assert not bad, (hex(flags), bad[:10])


# ------------------------------------------------------------------------------------------
# 1. 512 KiB compressed: landing decoder (inflate_seg3.h) and interval kernel (inflate_seg2.h)
# ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gate19(harness):
    """Noisy and half-zero ultra-fast streams of a little under 512 KiB, padded to 2^19 - 1, 2^19, 2^19 + 1 bytes."""
    names, blobs, raws = [], [], []
    for kind, sid in (("noisy", 0), ("halfzero", 7)):
        raw, comp = _scaled_to(lambda n: _bench(sid, n), ob.compress_ultra_fast, (1 << 19) - 1, 400000, 8192)
        assert _inflate_py(comp) == raw
        for tag, size in (("under", (1 << 19) - 1), ("at", 1 << 19), ("over", (1 << 19) + 1)):
            blob = harness.pad_to(comp, size)
            _oracle_pins_padding(blob, raw)
            names.append("%s_%s" % (kind, tag))
            blobs.append(blob)
            raws.append(raw)
    return names, blobs, raws


def test_gate_512k_compressed_padded_streams(harness, gate19):
    """The 2^19-byte gate of the landing decoder and the interval kernel (`ilen < 2^19`): input slots of 2^19 - 1, 2^19
    and 2^19 + 1 bytes.  Alone, either kernel leaves the streams at and over the gate PENDING and untouched.  Just under
    it neither takes noisy content of that length anyway (their check-point slots run out near 94 KB of noisy input:
    test_landing_and_interval_kernels_largest_noisy_stream), so for these two the gate has no "taken just under" side
    on such content -- what they do report under it must be right; the slot gate below has both sides.  The segment
    kernel and the lane kernel (gates at 2^28) take all six; the whole pipeline is bit-exact with every kernel in or
    out of the chain."""
    names, blobs, raws = gate19
    for slack in (0, 17):
        caps = [len(r) + slack for r in raws]
        for flags in (0, 0x400, 128, 1):
            _assert_whole(harness, names, blobs, caps, raws, flags)
        leave = [n for n in names if n.endswith(("_at", "_over"))]
        for flags in (LANDING_ONLY, INTERVAL_ONLY, LANDING_INTERVAL):
            _assert_alone(harness, names, blobs, caps, raws, flags, leave=leave)
        _assert_alone(harness, names, blobs, caps, raws, SEGMENT_ONLY, take=names)
    # the lane kernel takes 16-byte aligned slots only: one stream per call
    _assert_alone(harness, names, blobs, [len(r) for r in raws], raws, LANES_ONLY, take=names, one_by_one=True)


# measured on an MI355X, one stream per call in an exact slot (bench buffer 0: noisy rows, ~0.504 compressed bytes per byte)
LANDING_TAKES_NOISY = 186352    # 93 989 compressed bytes; 186 353 is passed on
INTERVAL_TAKES_NOISY = 188228   # 94 933 compressed bytes; 188 229 is passed on


def test_landing_and_interval_kernels_largest_noisy_stream(harness):
    """Where the landing decoder and the interval kernel stop taking noisy streams for reasons of their own (48
    check-point slots per lane, inflate_seg2.h:57-59): far below their 2^19 gate.  Pinned from both sides -- taken at
    N, passed on (PENDING, not wrong) at N + 1 -- so that a change that moves the hand-over shows here and not only as
    speed; the whole pipeline is exact on both sides."""
    for flags, n_take, who in ((LANDING_ONLY, LANDING_TAKES_NOISY, "landing decoder"),
                               (INTERVAL_ONLY, INTERVAL_TAKES_NOISY, "interval kernel"),
                               (LANDING_INTERVAL, INTERVAL_TAKES_NOISY, "landing decoder + interval kernel")):
        for n, taken in ((n_take, True), (n_take + 1, False), (400000, False), (1000000, False)):
            raw = _bench(0, n)
            comp = ob.compress_ultra_fast(raw)
            assert len(comp) < (1 << 19) and _inflate_py(comp) == raw
            st, ln, ad, slots, guards_ok = harness.gpu_inflate_big([comp], [n], flags=flags)
            print("%s: %d raw / %d compressed bytes -> %#x" % (who, n, len(comp), int(st[0])))
            assert guards_ok
            if taken:
                assert int(st[0]) == 0 and int(ln[0]) == n and int(ad[0]) == zlib.adler32(raw) and slots.head_equals(0, raw), (who, n)
            else:
                assert int(st[0]) == PENDING, (who, n, hex(int(st[0])))
            _assert_whole(harness, ["noisy%d" % n], [comp], [n], [raw])


@pytest.fixture(scope="module")
def long_uf():
    """Unpadded ultra-fast streams of 600 KB .. 15 MiB raw, noisy and half zero: five of the eight are 512 KiB compressed
    and more (the 600 KB ones and the half-zero MiB are shorter, and still too long for the two kernels in front)."""
    out = []
    for n in (600_000, 1 << 20, 4 << 20, 15 << 20):
        for kind, sid in (("noisy", 0), ("halfzero", 7)):
            raw = _bench(sid, n + (5 if kind == "halfzero" else 0))
            comp = ob.compress_ultra_fast(raw)
            if n == 1 << 20:
                assert _inflate_py(comp) == raw
            out.append(("%s%d" % (kind, n), comp, raw))
    assert sum(1 for _, c, _ in out if len(c) >= 1 << 19) == 5
    return out


def test_long_ultrafast_streams_exact_loose_short_slots_and_damage(harness, long_uf):
    """Ultra-fast streams of 512 KiB compressed and more -- an ordinary 1 MiB noisy scanline buffer is one -- through
    fdh_inflate_batch: exact, loose (+17, +33) and short (-1, half) slots, a cut, a mid-stream bit flip and a damaged
    trailer of each (the segment kernel must hand those to the exact kernels: the oracle's status and lengths), with
    the whole chain, without the interval kernel, without any segment-parallel kernel and with ignore_adler32."""
    r = np.random.default_rng(19)
    vn, vb, vc, vr = [], [], [], []      # valid, slot holds the stream
    on, ob_, oc = [], [], []             # the oracle decides
    for name, comp, raw in long_uf:
        for c in (len(raw), len(raw) + 17, len(raw) + 33):
            vn.append("%s@%d" % (name, c)); vb.append(comp); vc.append(c); vr.append(raw)
        for c in (len(raw) - 1, len(raw) // 2):
            on.append("%s@%d" % (name, c)); ob_.append(comp); oc.append(c)
        cut = int(r.integers(len(comp) // 2, len(comp) - 4))
        on.append("%s_cut%d" % (name, cut)); ob_.append(comp[:cut]); oc.append(len(raw))
        bad = bytearray(comp)
        bad[len(bad) // 2 + int(r.integers(0, 1000))] ^= 0x10
        on.append("%s_flip" % name); ob_.append(bytes(bad)); oc.append(len(raw) + 100)
        bad = bytearray(comp)
        bad[-2] ^= 0x01
        on.append("%s_adler" % name); ob_.append(bytes(bad)); oc.append(len(raw))
    for flags in (0, 0x400, 128, 1):
        _assert_whole(harness, vn, vb, vc, vr, flags)
        _assert_oracle(harness, on, ob_, oc, flags)
    _assert_alone(harness, vn, vb, vc, vr, SEGMENT_ONLY, take=vn)
    for flags in (LANDING_ONLY, INTERVAL_ONLY):   # too long for them whatever the gate says: nothing reported, or right
        _assert_alone(harness, vn, vb, vc, vr, flags)


# ------------------------------------------------------------------------------------------
# 2. 16 MiB slot: landing decoder and interval kernel (`ocap < 2^24`)
# ------------------------------------------------------------------------------------------

def test_gate_16m_slot_small_stream(harness):
    """A 64 KiB bench stream in slots of 2^24 - 1 (taken by the landing decoder, and by the interval kernel), 2^24 and
    2^24 + 1 bytes (PENDING, untouched): the pair that pins `ocap < 2^24` for both kernels.  The segment kernel and the
    lane kernel take all three; the whole pipeline is exact."""
    raw = _bench(0, 65536)
    comp = ob.compress_ultra_fast(raw)
    assert _inflate_py(comp) == raw
    caps = [(1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    names = ["slot%d" % c for c in caps]
    blobs, raws = [comp] * 3, [raw] * 3
    for flags in (0, 0x400, 128):
        _assert_whole(harness, names, blobs, caps, raws, flags)
    for flags in (LANDING_ONLY, INTERVAL_ONLY, LANDING_INTERVAL):
        _assert_alone(harness, names, blobs, caps, raws, flags, take=names[:1], leave=names[1:])
    _assert_alone(harness, names, blobs, caps, raws, SEGMENT_ONLY, take=names)
    _assert_alone(harness, names, blobs, caps, raws, LANES_ONLY, take=names, one_by_one=True)


def test_gate_16m_slot_output_that_long(harness):
    """Streams whose OUTPUT is 2^24 - 1, 2^24 and 2^24 + 16 bytes, zero-heavy so that the compressed side stays far
    under 512 KiB and only the slot gate decides: exact slots.  At and over the gate the landing decoder and the
    interval kernel leave them PENDING and untouched; under it they may take them or pass them on (right if reported);
    the segment kernel takes all of them.  Short slots (-1, half) against the oracle."""
    names, blobs, raws = [], [], []
    for n in ((1 << 24) - 1, 1 << 24, (1 << 24) + 16):
        for kind in ("zero", "sparse"):
            y = np.zeros(n, dtype=np.uint8)
            if kind == "sparse":
                y[::4099] = 1
            comp = ob.compress_ultra_fast(y)
            assert len(comp) < 1 << 19
            assert _inflate_py(comp) == y.tobytes()
            names.append("%s%d" % (kind, n)); blobs.append(comp); raws.append(y.tobytes())
    caps = [len(x) for x in raws]
    for flags in (0, 0x400, 128):
        _assert_whole(harness, names, blobs, caps, raws, flags)
    leave = [nm for nm, x in zip(names, raws) if len(x) >= 1 << 24]
    for flags in (LANDING_ONLY, INTERVAL_ONLY, LANDING_INTERVAL):
        _assert_alone(harness, names, blobs, caps, raws, flags, leave=leave)
    _assert_alone(harness, names, blobs, caps, raws, SEGMENT_ONLY, take=names)
    short = [c - 1 for c in caps] + [c // 2 for c in caps]
    _assert_oracle(harness, ["%s@%d" % (nm, c) for nm, c in zip(names * 2, short)], blobs * 2, short)


# ------------------------------------------------------------------------------------------
# 3. / 4. 128 MiB compressed (LZ-window kernel, resume records), 256 MiB compressed (segment / lane kernel)
# ------------------------------------------------------------------------------------------

def _skewed(n, seed):
    """Random bytes of a 200-letter alphabet: 7.64 bits a byte, so zlib writes Huffman blocks (bytes that use all 256
    values do not compress, and zlib then stores them whatever the strategy -- the stored stream is a case of its own)."""
    return np.random.default_rng(seed).integers(0, 200, n, dtype=np.uint8).tobytes()


def _huffman_only(raw):
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    return c.compress(raw) + c.flush()


@pytest.fixture(scope="module")
def big_general():
    """Built once, in threads (zlib releases the GIL): Huffman-only zlib streams of a little under 2^27 bytes and of
    2^27 + ~1.2 MiB real bytes, and a stored (level 0) stream of 2^27 raw bytes."""
    t0 = time.time()
    probe = _skewed(8 << 20, 3)
    ratio = len(_huffman_only(probe)) / len(probe)
    n_under = int(((1 << 27) - 300_000) / ratio)
    n_over = int(((1 << 27) + 1_300_000) / ratio)
    with ThreadPoolExecutor(4) as pool:
        f_raw_u = pool.submit(_skewed, n_under, 5)
        f_raw_o = pool.submit(_skewed, n_over, 6)
        f_raw_s = pool.submit(lambda: np.random.default_rng(7).integers(0, 256, 1 << 27, dtype=np.uint8).tobytes())
        raw_u, raw_o, raw_s = f_raw_u.result(), f_raw_o.result(), f_raw_s.result()
        f_u, f_o, f_s = pool.submit(_huffman_only, raw_u), pool.submit(_huffman_only, raw_o), pool.submit(zlib.compress, raw_s, 0)
        comp_u, comp_o, comp_s = f_u.result(), f_o.result(), f_s.result()
        assert (1 << 27) - 600_000 < len(comp_u) < (1 << 27) - 1, len(comp_u)
        assert (1 << 27) + (1 << 20) + 1000 < len(comp_o) < (1 << 27) + (2 << 20), len(comp_o)
        assert len(comp_s) >= 1 << 27
        for f in [pool.submit(lambda b, r: _inflate_py(b) == r, b, r) for b, r in ((comp_u, raw_u), (comp_o, raw_o), (comp_s, raw_s))]:
            assert f.result()
    print("big_general built in %.1f s: %d / %d / %d compressed bytes" % (time.time() - t0, len(comp_u), len(comp_o), len(comp_s)))
    return dict(raw_u=raw_u, comp_u=comp_u, raw_o=raw_o, comp_o=comp_o, raw_s=raw_s, comp_s=comp_s)


def test_gate_128m_compressed_lz_window_kernel(harness, big_general):
    """The LZ-window kernel takes a stream of 8 <= bytes < 2^27 (30-bit bit positions): a Huffman-only zlib stream
    padded to 2^27 - 1 bytes is finished by it alone (FDH_FLAG_LZ_ONLY); at 2^27, 2^27 + 1 and with 2^27 + 1.2 MiB of
    real stream it is left (PENDING*) with the slot untouched, and the whole pipeline -- the exact kernels, which start
    such a stream at its first byte: a resume record keeps no bit position of 2^30 and more -- is bit-exact on all of
    them and on a stored stream of the same size."""
    _need(3 << 30, "128 MiB streams")
    g = big_general
    names = ["under", "at", "over", "real_over", "stored"]
    blobs = [harness.pad_to(g["comp_u"], (1 << 27) - 1), harness.pad_to(g["comp_u"], 1 << 27), harness.pad_to(g["comp_u"], (1 << 27) + 1),
             g["comp_o"], g["comp_s"]]
    raws = [g["raw_u"]] * 3 + [g["raw_o"], g["raw_s"]]
    with ThreadPoolExecutor(3) as pool:   # the padding changes nothing for the oracle
        assert all(pool.map(_oracle_decodes, blobs[:3], raws[:3]))
    caps = [len(r) for r in raws]
    _assert_alone(harness, names, blobs, caps, raws, LZ_ONLY, take=["under"], leave=["at", "over", "real_over"], pend_min=PENDING_ANY)
    for i, name in enumerate(names):   # one call each: the wall time of a stream is that of the kernel that took it
        t0 = time.time()
        _assert_whole(harness, [name], [blobs[i]], [caps[i]], [raws[i]])
        print("whole pipeline, %s (%d compressed bytes): %.2f s" % (name, len(blobs[i]), time.time() - t0))


def test_gate_128m_compressed_cut_streams(harness, big_general):
    """Cut at a random byte of the last MiB: InsufficientInput with the oracle's partial length and bytes.  The cut of
    the stream under 2^27 bytes is re-derived from the LZ-window kernel's check point; the one over 2^27 bytes has none
    (bit positions of 2^30 and more do not fit a record) and is decoded from its first byte -- FDH_FLAG_NO_CHECKPOINTS
    must give the same for both."""
    _need(3 << 30, "128 MiB streams")
    g = big_general
    r = np.random.default_rng(27)
    names, blobs, caps = [], [], []
    for tag in ("u", "o"):
        comp, raw = g["comp_" + tag], g["raw_" + tag]
        cut = len(comp) - 1 - int(r.integers(0, 1 << 20))
        if tag == "o":
            assert cut >= 1 << 27
        names.append("cut_%s_%d" % (tag, cut)); blobs.append(comp[:cut]); caps.append(len(raw))
    for flags in (0, NO_CHECKPOINTS):
        t0 = time.time()
        _assert_oracle(harness, names, blobs, caps, flags)
        print("cut streams, flags %#x: %.2f s (oracle included)" % (flags, time.time() - t0))


@pytest.fixture(scope="module")
def big_uf():
    """Noisy ultra-fast streams (bench rows, generated on the device 4 MiB a buffer) of a little under 2^28 compressed
    bytes and of a little over."""
    from fdeflate_amd import synth
    t0 = time.time()
    raw_all = synth.gen_batch_torch(100, 160, 4 << 20, device="cuda", chunk=4).view(-1).cpu().numpy()

    def fit(lo, hi):
        """The prefix of raw_all whose stream is lo .. hi bytes long (the 4 MiB buffers differ: zero, half zero, noisy)."""
        n = int(raw_all.size * 0.9)
        for _ in range(6):
            comp = ob.compress_ultra_fast(raw_all[:n])
            if lo <= len(comp) <= hi:
                return n, comp
            n = int(n * ((lo + hi) / 2) / len(comp))
            assert n <= raw_all.size, n
        raise AssertionError("no prefix with a stream of %d .. %d bytes" % (lo, hi))

    with ThreadPoolExecutor(2) as pool:
        (n_under, comp_u), (n_over, comp_o) = pool.map(lambda r: fit(*r), (((1 << 28) - 800_000, (1 << 28) - 2),
                                                                          (1 << 28, (1 << 28) + 800_000)))
        ok_u, ok_o = pool.map(lambda b_n: _inflate_py(b_n[0]) == raw_all[:b_n[1]].tobytes(), ((comp_u, n_under), (comp_o, n_over)))
        assert ok_u and ok_o
    print("big_uf built in %.1f s: %d / %d compressed bytes" % (time.time() - t0, len(comp_u), len(comp_o)))
    return dict(raw_u=raw_all[:n_under], comp_u=comp_u, raw_o=raw_all[:n_over], comp_o=comp_o)


def test_gate_256m_compressed_segment_and_lane_kernels(harness, big_uf):
    """The segment kernel and the lane kernel take `ilen < 2^28` (31-bit bit positions): a noisy ultra-fast stream
    padded to 2^28 - 1 bytes is finished by either alone; padded to 2^28 and with 2^28 real bytes and more it is left
    PENDING, untouched, and the exact kernels take it.  The whole pipeline is bit-exact on all."""
    _need(4 << 30, "256 MiB streams")
    g = big_uf
    names = ["under", "at", "real_over"]
    blobs = [harness.pad_to(g["comp_u"], (1 << 28) - 1), harness.pad_to(g["comp_u"], 1 << 28), g["comp_o"]]
    raws = [g["raw_u"], g["raw_u"], g["raw_o"]]
    with ThreadPoolExecutor(2) as pool:
        assert all(pool.map(_oracle_decodes, blobs[:2], raws[:2]))   # the padding changes nothing for the oracle
    caps = [len(r) for r in raws]
    for flags, one in ((SEGMENT_ONLY, False), (LANES_ONLY, True)):
        t0 = time.time()
        _assert_alone(harness, names, blobs, caps, raws, flags, take=["under"], leave=["at", "real_over"], one_by_one=one)
        print("flags %#x on the 256 MiB streams: %.2f s" % (flags, time.time() - t0))
    for i, name in enumerate(names):
        t0 = time.time()
        _assert_whole(harness, [name], [blobs[i]], [caps[i]], [raws[i]])
        print("whole pipeline, %s (%d compressed bytes): %.2f s" % (name, len(blobs[i]), time.time() - t0))


def test_gate_2_31_stream_bits_span_decoder(harness, big_general):
    """The span decoder (FDH_FLAG_SPANS 0x100, inside the 12-bit general kernel) takes `stream bits < 2^31`, counted
    over the whole input slot: the Huffman-only stream of 2^27 + 1.2 MiB real bytes padded to 2^28 - 1, 2^28 and
    2^28 + 1 bytes.  With 0x100 | 0x200 (no small-table kernel in front; the LZ-window kernel's own gate keeps it out)
    the 12-bit kernel gets all three, with its span decoder under the gate and without it at and over.  There is no
    flag that runs the span decoder alone or reports who decoded, so what is pinned is that both sides are bit-exact."""
    _need(4 << 30, "256 MiB input slots")
    g = big_general
    sizes = [(1 << 28) - 1, 1 << 28, (1 << 28) + 1]
    names = ["bits_under", "bits_at", "bits_over"]
    blobs = [harness.pad_to(g["comp_o"], n) for n in sizes]
    raws = [g["raw_o"]] * 3
    with ThreadPoolExecutor(3) as pool:
        assert all(pool.map(_oracle_decodes, blobs, raws))   # the padding changes nothing for the oracle
    for flags in (0x100 | 0x200, 0x100):
        for i, name in enumerate(names):
            t0 = time.time()
            _assert_whole(harness, [name], [blobs[i]], [len(raws[i])], [raws[i]], flags)
            print("flags %#x, %s (%d bytes of input slot): %.2f s" % (flags, name, sizes[i], time.time() - t0))


# ------------------------------------------------------------------------------------------
# 5. 1 GiB and 2 GiB slots
# ------------------------------------------------------------------------------------------

GIB_SLOTS = [(1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, 0xFFFFFFF0]


@pytest.mark.parametrize("cap", GIB_SLOTS)
def test_gate_gib_slots_short_streams(harness, cap):
    """A short zlib-6 stream and a short ultra-fast stream in slots of 2^30 - 1 .. 0xFFFFFFF0 bytes: the LZ-window
    kernel takes `16 <= cap < 2^30`, the segment and the lane kernel `ocap < 2^31`, the span decoder (flag 0x100)
    `cap < 2^31`; the exact kernels clamp the capacity to 0xFFFFFFFF.  Alone, each kernel finishes the stream under its
    gate and leaves it PENDING, untouched, at and over; the whole pipeline (also with the span decoder) is exact."""
    _need(2 * cap + (2 << 30), "two slots of %d bytes" % cap)
    raw = _bench(3, 65536)
    z6 = zlib.compress(raw, 6)
    uf = ob.compress_ultra_fast(raw)
    assert _inflate_py(uf) == raw
    names, blobs, raws, caps = ["zlib6", "uf"], [z6, uf], [raw, raw], [cap, cap]
    for flags in (0, 0x100, 128):
        _assert_whole(harness, names, blobs, caps, raws, flags)
    lz_takes = cap < 1 << 30
    _assert_alone(harness, names[:1], blobs[:1], caps[:1], raws[:1], LZ_ONLY, take=names[:1] if lz_takes else (),
                  leave=() if lz_takes else names[:1], pend_min=PENDING_ANY)
    seg_takes = cap < 1 << 31
    for flags in (SEGMENT_ONLY, LANES_ONLY):
        _assert_alone(harness, names[1:], blobs[1:], caps[1:], raws[1:], flags, take=names[1:] if seg_takes else (),
                      leave=() if seg_takes else names[1:])


TAIL = 4 << 20   # the "tail" buffers end this far behind 2^30 + 5 / 2^31 + 5 bytes


@pytest.fixture(scope="module", params=[(1 << 30) + 5, (1 << 31) + 5])
def gib_outputs(request):
    """Buffers of 2^30 + 5 or 2^31 + 5 bytes (one size alive at a time), built once, in threads: all-zero and sparse (y[::4099] = 1) as ultra-fast
    streams, all-zero as a zlib-6 stream, and for zlib-6 a "tail" buffer that is 4 MiB longer: zeros up to 2 MiB in
    front of 2^30 + 5 / 2^31 + 5, then the sparse pattern across that position (258-byte matches at distance 4099)
    and, in the last MiB, a random block of 32 000 bytes over and over (matches at distance 32 000)."""
    t0 = time.time()

    def make(n, kind):
        y = np.zeros(n + (TAIL if kind == "tail" else 0), dtype=np.uint8)
        if kind == "sparse":
            y[::4099] = 1
        if kind == "tail":
            y[n - (2 << 20)::4099] = 1
            block = np.random.default_rng(n & 0xFFFF).integers(0, 256, 32000, dtype=np.uint8)
            y[-(1 << 20):] = np.resize(block, 1 << 20)
        return y

    def z6(y):
        c = zlib.compressobj(6)
        parts = [c.compress(y[o:o + (1 << 28)]) for o in range(0, y.size, 1 << 28)]
        return b"".join(parts) + c.flush()

    wanted = {"zero": ("uf", "z6"), "sparse": ("uf",), "tail": ("z6",)}
    out = {}
    with ThreadPoolExecutor(8) as pool:
        ys = {(n, k): pool.submit(make, n, k) for n in (request.param,) for k in wanted}
        ys = {key: f.result() for key, f in ys.items()}
        fs = {}
        for key, y in ys.items():
            for fmt in wanted[key[1]]:
                fs[key + (fmt,)] = pool.submit(ob.compress_ultra_fast if fmt == "uf" else z6, y)
            fs[key + ("adler",)] = pool.submit(zlib.adler32, y)
        for key, f in fs.items():
            out[key] = f.result()
    for key, y in ys.items():
        out[key + ("raw",)] = y
    out["n"] = request.param
    print("gib_outputs %d built in %.1f s" % (request.param, time.time() - t0))
    return out


@pytest.mark.parametrize("fmt", ["uf", "z6"])
def test_output_of_a_gib_and_more(harness, gib_outputs, fmt):
    """Output that really is 2^30 + 5 / 2^31 + 5 bytes long (over the LZ-window kernel's and the segment / lane / span
    kernels' slot gates): exact slot -> Ok with the buffer's length, bytes and Adler-32; slot - 1 -> OutputTooLarge,
    length = capacity, the slot holds the prefix.  Ultra-fast: all-zero and sparse buffers.  zlib-6: the all-zero buffer
    and the "tail" buffer, whose matches at distances 4099 and 32 000 lie either side of output position 2^30 + 5 /
    2^31 + 5 -- the exact kernels' back-references (ring and far copies from the slot) at those positions.

    The zlib-6 stream of the buffer that is sparse from its FIRST byte is not decoded at these sizes: behind the
    LZ-window kernel (which the slot gate keeps out) the exact kernels take its 258-byte matches at distance 4099 at
    1.6 - 2 MB/s once the output has passed a few MiB (measured: 4 MiB 53 MB/s, 16 MiB 2.0 MB/s, 64 MiB 1.6 MB/s; the
    all-zero stream 47 MB/s at every size), i.e. eleven minutes for 2^30 + 5 bytes and twice that for 2^31 + 5
    (DESIGN.md "Size gates").  The tail buffer pays that rate for 6 MiB, and puts the same matches where the gate is."""
    n = gib_outputs["n"]
    _need(2 * n + (3 << 30), "two slots of %d bytes" % n)
    for kind in ("zero", "sparse") if fmt == "uf" else ("zero", "tail"):
        y, blob, adler = gib_outputs[(n, kind, "raw")], gib_outputs[(n, kind, fmt)], gib_outputs[(n, kind, "adler")]
        m = y.size
        if kind in ("sparse", "tail"):   # (the encoder stays out of the expectation; once per format and size is enough)
            d = zlib.decompressobj()
            got = 0
            for o in range(0, len(blob), 1 << 16):
                piece = d.decompress(blob[o:o + (1 << 16)])
                assert piece == y[got:got + len(piece)].tobytes()
                got += len(piece)
            assert got == m
        t0 = time.time()
        st, ln, ad, slots, guards_ok = harness.gpu_inflate_big([blob, blob], [m, m - 1])
        print("%s %s %d: %.2f s" % (fmt, kind, m, time.time() - t0))
        assert guards_ok
        assert int(st[0]) == 0 and int(ln[0]) == m and int(ad[0]) == adler, (kind, hex(int(st[0])), int(ln[0]), hex(int(ad[0])))
        assert slots.head_equals(0, y), kind
        assert int(st[1]) == 17 and int(ln[1]) == m - 1, (kind, hex(int(st[1])), int(ln[1]))
        assert slots.head_equals(1, y[:m - 1]), kind


# ------------------------------------------------------------------------------------------
# 6. one mixed batch
# ------------------------------------------------------------------------------------------

def test_mixed_batch_streams_from_both_sides_of_every_gate(harness, gate19, long_uf, big_general, big_uf):
    """One stream from each side of each gate next to 300 ordinary 64 KiB streams in ONE call, flags 0: lists, hand-out
    counters and the side stream see big and small streams together.  Bit-exact."""
    _need(6 << 30, "the mixed batch")
    names, blobs, caps, raws = [], [], [], []

    def add(name, blob, raw, cap=None):
        names.append(name); blobs.append(blob); raws.append(raw); caps.append(len(raw) if cap is None else cap)

    gn, gb, gr = gate19
    for i in (0, 2, 3, 4):
        add("c19_" + gn[i], gb[i], gr[i])
    small = _bench(0, 65536)
    small_c = ob.compress_ultra_fast(small)
    z6 = zlib.compress(small, 6)
    add("slot24_under", small_c, small, (1 << 24) - 1)
    add("slot24_at", small_c, small, 1 << 24)
    add("slot30_under", z6, small, (1 << 30) - 1)
    add("slot30_at", z6, small, 1 << 30)
    add("slot31_under", small_c, small, (1 << 31) - 1)
    add("slot31_at", small_c, small, 1 << 31)
    add("c27_under", harness.pad_to(big_general["comp_u"], (1 << 27) - 1), big_general["raw_u"])
    add("c27_over", big_general["comp_o"], big_general["raw_o"])
    add("c27_stored", big_general["comp_s"], big_general["raw_s"])
    add("c28_under", harness.pad_to(big_uf["comp_u"], (1 << 28) - 1), big_uf["raw_u"])
    add("c28_over", big_uf["comp_o"], big_uf["raw_o"])
    for name, comp, raw in long_uf[:4]:
        add(name, comp, raw)
    for k in range(300):
        raw = _bench(200 + k, 65536)
        if k % 3 == 0:
            add("z6_%d" % k, zlib.compress(raw, 6), raw)
        else:
            add("uf_%d" % k, ob.compress_ultra_fast(raw), raw)
    order = np.random.default_rng(6).permutation(len(names))
    t0 = time.time()
    _assert_whole(harness, [names[i] for i in order], [blobs[i] for i in order], [caps[i] for i in order], [raws[i] for i in order])
    print("mixed batch of %d streams: %.2f s" % (len(names), time.time() - t0))


# ------------------------------------------------------------------------------------------
# 7. encoders: slots that are too small
# ------------------------------------------------------------------------------------------

def _encoder_inputs():
    from fdeflate_amd import synth
    r = np.random.default_rng(41)
    raws = [b"", b"a", bytes(1), bytes(7), bytes(8), bytes(9), b"Hello world!", bytes(300), bytes([7]) * 300]
    for n in (15, 16, 17, 63, 64, 65, 511, 512, 513, 1000, 4096, 20000, 65536, 70001):
        x = r.integers(0, 256, n, dtype=np.uint8)
        raws.append(x.tobytes())
        y = x.copy()
        y[r.random(n) < 0.8] = 0
        raws.append(y.tobytes())
    for sid in (0, 7, 15):
        raws.append(synth.gen_stream_np(sid, 65536).tobytes())
    raws.append(bytes(3_000_000))                            # one run: the bit ring's slow path
    raws.append(bytes(3_000_000) + b"\x07" + bytes(100))
    raws.append(bytes(1_500_000) + b"\x07" + bytes(1_500_000))
    return raws


def _overflow_caps(want, bound):
    """Every third slot too small -- by 1 byte, by half, 1 byte long, 0 bytes long in turn --, the others exactly the
    compressed length (the header asks for the bound; the code checks the bytes) or the bound."""
    caps, small = [], []
    for i, w in enumerate(want):
        if i % 3 == 1:
            c = (len(w) - 1, len(w) // 2, 1, 0)[(i // 3) % 4]
            caps.append(c); small.append(True)
        else:
            caps.append(len(w) if i % 3 == 0 else bound(i))
            small.append(False)
    return caps, small


def _assert_encoder_slots(tag, ln, slots, guards_ok, want, small, fill):
    """guards_ok: the list of guard-slot faults (empty: none)."""
    assert not guards_ok, (tag, guards_ok[:8])
    for i, w in enumerate(want):
        if small[i]:
            assert int(ln[i]) == 0xFFFFFFFF, (tag, i, len(w), slots[i].size, int(ln[i]))
            continue
        assert int(ln[i]) == len(w), (tag, i, int(ln[i]), len(w), slots[i].size)
        assert slots[i][:len(w)].tobytes() == w, (tag, i, "not bit-exact next to an overflowing neighbour")
        assert np.all(slots[i][len(w):] == fill), (tag, i, "wrote behind its stream")


def test_ultrafast_encoder_slots_too_small(harness):
    """fdh_deflate_ultrafast_batch with every third slot too small, at odd alignments, guard slots in between:
    out_len = 0xFFFFFFFF for exactly those, no byte outside any slot changed (guard slots: an empty input's stream and
    3 or 16 bytes that nobody may write),
    every other stream bit-exact with the oracle; a slot of exactly the compressed length succeeds."""
    import fdeflate_amd as fd
    raws = _encoder_inputs()
    want = [ob.compress_ultra_fast(x) for x in raws]
    caps, small = _overflow_caps(want, lambda i: fd.ultrafast_bound(len(raws[i])))
    for guard in (3, 16):
        ln, slots, guards_ok = harness.gpu_encode_slots(fd.deflate_ultrafast_batch, raws, caps, ob.compress_ultra_fast(b""), guard=guard)
        _assert_encoder_slots("ultrafast guard %d" % guard, ln, slots, guards_ok, want, small, 0x5A)


@pytest.mark.parametrize("lanes", [None, "1", "64"])
def test_general_encoder_slots_too_small(harness, lanes, monkeypatch):
    """fdh_deflate_general_batch, level 1 and RLE, parser with FDH_GEN_LANES unset, 1 and 64: as above, plus 4.5 MiB of
    random bytes (the ring is flushed in the middle of a block) in a slot that is too small by one byte and in one of
    exactly the compressed length."""
    import fdeflate_amd as fd
    if lanes is None:
        monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    else:
        monkeypatch.setenv("FDH_GEN_LANES", lanes)
    raws = _encoder_inputs()
    big = np.random.default_rng(23).integers(0, 256, 4_718_592 + 11, dtype=np.uint8).tobytes()
    raws = raws[:4] + [big, big] + raws[4:]     # index 4: exact slot (4 % 3 == 1 would be small: see below), 5: too small
    for mode, enc in ((fd.MODE_LEVEL1, ob.compress_level1), (fd.MODE_RLE, ob.compress_rle)):
        want = [enc(x) for x in raws]
        caps, small = _overflow_caps(want, lambda i: fd.compress_bound(len(raws[i])))
        caps[4], small[4] = len(want[4]), False
        caps[5], small[5] = len(want[5]) - 1, True
        ln, slots, guards_ok = harness.gpu_encode_slots(
            lambda a, b, c, d: fd.deflate_general_batch(a, b, c, d, mode), raws, caps, enc(b""))
        _assert_encoder_slots("general mode %d lanes %s" % (mode, lanes), ln, slots, guards_ok, want, small, 0x5A)


def test_png_fused_encoder_slots_too_small(harness):
    """fdh_png_filter_deflate_ultrafast_batch shares the ultra-fast encoder's tail: a slot that is too small gives
    out_len = 0xFFFFFFFF with png_status 0 (include/fdeflate_hip.h), nothing outside the slot changes, the neighbours
    are bit-exact with the oracle's filter + ultra-fast encoder."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(43)
    for rb, bpp in ((1, 1), (21, 3), (1024, 4), (1000, 8)):
        images = []
        for rows in (0, 1, 2, 5, 64, 257, 64, 3, 700, 1, 64, 64):
            pix = r.integers(0, 256, rows * rb, dtype=np.uint8)
            pix[r.random(rows * rb) < 0.5] = 0
            if rows >= 64:
                pix[rb * 2:rb * 40] = 0
            images.append((pix.tobytes(), bytes(r.integers(0, 5, rows, dtype=np.uint8))))
        images.append((bytes(rb * 3000), bytes(3000)))     # all zero: long runs
        want = []
        for pix, types in images:
            est, filt = ob.png_filter(pix, rb, bpp, types)
            assert est == 0
            want.append(ob.compress_ultra_fast(filt))
        caps, small = _overflow_caps(want, lambda i: fd.ultrafast_bound(len(images[i][1]) * (rb + 1)))
        fill, guard, empty = 0xEE, 3, ob.compress_ultra_fast(b"")
        all_pix, all_types, all_caps = [], [], []
        for (pix, types), c in zip(images, caps):
            all_pix += [pix, b""]; all_types += [types, b""]; all_caps += [c, len(empty) + guard]
        pbuf, poff = streams.pack_exact(all_pix)
        tbuf, toff = streams.pack_exact(all_types)
        ooff = np.zeros(len(all_caps) + 1, dtype=np.int64)
        ooff[1:] = np.cumsum(all_caps)
        d_out = torch.full((int(ooff[-1]),), fill, dtype=torch.uint8, device="cuda")
        ol, st = fd.png_filter_deflate_ultrafast_batch(
            torch.from_numpy(pbuf).cuda(), torch.from_numpy(poff.astype(np.int64)).cuda(), torch.from_numpy(tbuf).cuda(),
            torch.from_numpy(toff.astype(np.int64)).cuda(), d_out, torch.from_numpy(ooff).cuda(), rb, bpp)
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        ln = ol.cpu().numpy().view(np.uint32)
        assert not st.cpu().numpy().any(), ("png_status", rb, bpp)   # an overflowing slot is no PNG error
        n = len(images)
        slots = [h[int(ooff[2 * i]):int(ooff[2 * i + 1])] for i in range(n)]
        _assert_encoder_slots("png rb %d bpp %d" % (rb, bpp), ln[0::2], slots, harness.encoder_guard_faults(h, ooff, ln, empty, fill), want, small, fill)


def test_png_fused_encoder_gate_two_gib_of_filtered_bytes(harness):
    """fdh_png_filter_deflate_ultrafast_batch takes an image only if rows < Q = 2^31 / (row_bytes + 1), rounded down (its
    filtered offsets are 32-bit, PngSource::divide multiplies them by floor(2^32 / (row_bytes + 1))).  Rows of 4092 bytes
    (row_bytes + 1 = 4093: a row's start falls on every phase of the encoder's 8-byte chunks), bpp 4, random filter
    types; one batch holds a small image, one of Q - 1 rows, one of Q rows and another small one, guard slots between them.
    Q - 1 rows: png_status 0, the stream bit for bit the oracle's filter + ultra-fast encoder in a slot of its length + 5,
    and decoded back on the GPU it is the filtered image, its length and its Adler-32.  The pixels are zero but for three
    stretches of noisy rows -- at the start, either side of filtered offset 2^30 and in the last MiB --, so `divide`
    works on offsets up to 2^31 while host time and stream size stay small.  Q rows: png_status 2, out_len 0, its slot
    and the guard slots keep their bytes."""
    import torch
    import fdeflate_amd as fd
    _need(12 << 30, "two 2 GiB images, the decoded copy and the comparison")
    t0 = time.time()
    rb, bpp, fill = 4092, 4, 0x5A
    q = (1 << 31) // (rb + 1)
    assert q * (rb + 1) <= (1 << 31) < (q + 1) * (rb + 1)
    r = np.random.default_rng(59)
    rows = q - 1
    pix = np.zeros((rows, rb), dtype=np.uint8)
    mid = (1 << 30) // (rb + 1)
    for lo, hi in ((0, 256), (mid - 128, mid + 128), (rows - 256, rows)):
        noise = r.integers(0, 256, (hi - lo, rb), dtype=np.uint8)
        noise[r.random(noise.shape) < 0.4] = 0
        pix[lo:hi] = noise
    types = r.integers(0, 5, rows, dtype=np.uint8)
    est, filt = ob.png_filter(pix.reshape(-1), rb, bpp, types)
    assert est == 0 and len(filt) == rows * (rb + 1) and (1 << 31) - 2 * (rb + 1) <= len(filt) < (1 << 31)
    want_big = ob.compress_ultra_fast(filt)
    t1 = time.time()
    smalls = []
    for nr in (70, 3):
        p = r.integers(0, 256, nr * rb, dtype=np.uint8)
        t = r.integers(0, 5, nr, dtype=np.uint8)
        smalls.append((p, t, ob.compress_ultra_fast(ob.png_filter(p, rb, bpp, t)[1])))
    empty = ob.compress_ultra_fast(b"")
    # [small, guard, Q - 1 rows, guard, Q rows, guard, small]; the guards are empty images
    nrows = [70, 0, rows, 0, q, 0, 3]
    poff = np.cumsum([0] + [n * rb for n in nrows]).astype(np.int64)
    toff = np.cumsum([0] + nrows).astype(np.int64)
    d_pix = torch.zeros(int(poff[-1]), dtype=torch.uint8, device="cuda")
    d_types = torch.zeros(int(toff[-1]), dtype=torch.uint8, device="cuda")     # (the image of Q rows: zeros, type 0)
    for slot, (p, t) in ((0, smalls[0][:2]), (2, (pix.reshape(-1), types)), (6, smalls[1][:2])):
        for c in range(0, p.size, 1 << 28):
            piece = p[c:c + (1 << 28)]
            d_pix[int(poff[slot]) + c:int(poff[slot]) + c + piece.size] = torch.from_numpy(piece.copy()).cuda()
        d_types[int(toff[slot]):int(toff[slot]) + t.size] = torch.from_numpy(t).cuda()
    del pix
    g = len(empty) + 3
    caps = [len(smalls[0][2]), g, len(want_big) + 5, g, 4096 + 5, g, len(smalls[1][2]) + 7]
    ooff = np.zeros(8, dtype=np.int64)
    ooff[1:] = np.cumsum(caps)
    d_out = torch.full((int(ooff[-1]),), fill, dtype=torch.uint8, device="cuda")
    ol, st = fd.png_filter_deflate_ultrafast_batch(d_pix, torch.from_numpy(poff).cuda(), d_types, torch.from_numpy(toff).cuda(),
                                                   d_out, torch.from_numpy(ooff).cuda(), rb, bpp)
    torch.cuda.synchronize()
    t2 = time.time()
    ln = ol.cpu().numpy().view(np.uint32)
    h = d_out.cpu().numpy()
    assert st.cpu().tolist() == [0, 0, 0, 0, 2, 0, 0], st.cpu().tolist()
    assert not harness.encoder_guard_faults(h, ooff, ln, empty, fill)
    assert int(ln[4]) == 0 and np.all(h[ooff[4]:ooff[5]] == fill), ("Q rows", int(ln[4]))
    for i, w in ((0, smalls[0][2]), (2, want_big), (6, smalls[1][2])):
        assert int(ln[i]) == len(w), (i, int(ln[i]), len(w))
        assert h[ooff[i]:ooff[i] + len(w)].tobytes() == w, (i, "not bit-exact")
        assert np.all(h[ooff[i] + len(w):ooff[i + 1]] == fill), (i, "wrote behind its stream")
    del d_pix, d_types, d_out
    dst, dl, ad, slots, guards_ok = harness.gpu_inflate_big([want_big], [len(filt)])
    assert guards_ok and int(dst[0]) == 0 and int(dl[0]) == len(filt) and int(ad[0]) == zlib.adler32(filt)
    assert slots.head_equals(0, filt)
    print("Q = %d rows of %d bytes: oracle %.1f s, %d compressed bytes, encode call %.1f s, whole test %.1f s"
          % (q, rb, t1 - t0, len(want_big), t2 - t1, time.time() - t0))


# ------------------------------------------------------------------------------------------
# 8. encoders: inputs that are too long
# ------------------------------------------------------------------------------------------

def test_general_encoder_gate_one_gib(harness):
    """The general encoder takes `len <= 2^30` (write_data splits above: src/compress/mod.rs:130-136).  Sparse buffers
    (zeros, a literal every 4099th byte) of 2^30 - 1 and 2^30 bytes are encoded bit for bit like the oracle's level 1 /
    RLE -- in slots of the compressed length + 7, the header's bound being 1.5 GiB --, one of 2^30 + 1 bytes gives
    out_len = 0xFFFFFFFF, all three in one batch between two ordinary buffers; the guard slots keep their bytes and
    the neighbours are bit-exact."""
    import torch
    import fdeflate_amd as fd
    _need(16 << 30, "three 1 GiB inputs and the encoder's records")
    r = np.random.default_rng(47)
    a = r.integers(0, 64, 70001, dtype=np.uint8).tobytes()
    b = bytes(5000) + b"abcabcabc" * 300
    sizes = [(1 << 30) - 1, 1 << 30, (1 << 30) + 1]
    lens = [len(a), 0, sizes[0], 0, sizes[1], 0, sizes[2], 0, len(b)]
    in_off = np.cumsum([0] + lens).astype(np.int64)
    d_in = torch.zeros(int(in_off[-1]), dtype=torch.uint8, device="cuda")
    d_in[:len(a)] = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).cuda()
    d_in[int(in_off[8]):] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    for k in (2, 4, 6):
        d_in[int(in_off[k]):int(in_off[k + 1])][::4099] = 1
    y = np.zeros(1 << 30, dtype=np.uint8)
    y[::4099] = 1
    for mode, enc in ((fd.MODE_LEVEL1, ob.compress_level1), (fd.MODE_RLE, ob.compress_rle)):
        want = {0: enc(a), 2: enc(y[:sizes[0]]), 4: enc(y), 8: enc(b)}
        assert zlib.decompress(want[4]) == y.tobytes()
        empty = enc(b"")
        g = len(empty) + 3
        caps = [len(want[0]), g, len(want[2]) + 7, g, len(want[4]) + 7, g, 4096 + 5, g, fd.compress_bound(len(b))]
        out_off = np.zeros(10, dtype=np.int64)
        out_off[1:] = np.cumsum(caps)
        d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
        t0 = time.time()
        ln = fd.deflate_general_batch(d_in, torch.from_numpy(in_off).cuda(), d_out, torch.from_numpy(out_off).cuda(), mode)
        ln = ln.cpu().numpy().view(np.uint32)
        print("general encoder, mode %d, 2^30 - 1 / 2^30 / 2^30 + 1 bytes in one batch: %.1f s" % (mode, time.time() - t0))
        h = d_out.cpu().numpy()
        assert int(ln[6]) == 0xFFFFFFFF, (mode, ln)
        assert not harness.encoder_guard_faults(h, out_off, ln, empty, 0x5A), mode
        for i, w in want.items():
            assert int(ln[i]) == len(w), (mode, i, int(ln[i]), len(w))
            assert h[out_off[i]:out_off[i] + len(w)].tobytes() == w, (mode, i)
            assert np.all(h[out_off[i] + len(w):out_off[i + 1]] == 0x5A), (mode, i)


def _uf_neighbours():
    r = np.random.default_rng(53)
    a = r.integers(0, 256, 70001, dtype=np.uint8)
    a[r.random(a.size) < 0.6] = 0
    return a.tobytes(), bytes(40000) + b"\x09" + bytes(13)


def _uf_batch_around(big_len, fill_big):
    """Device input [a | big | b] with the middle buffer filled in place by fill_big(view) -> (d_in, in_off, view)."""
    import torch
    a, b = _uf_neighbours()
    d_in = torch.zeros(len(a) + big_len + len(b), dtype=torch.uint8, device="cuda")
    d_in[:len(a)] = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).cuda()
    d_in[len(a) + big_len:] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    view = d_in[len(a):len(a) + big_len]
    fill_big(view)
    in_off = np.cumsum([0, len(a), 0, big_len, 0, len(b)]).astype(np.int64)
    return d_in, in_off, view


def _uf_encode_around(harness, d_in, in_off, big_cap):
    """Encodes [a, guard, big, guard, b] -> (out_len, host copy of the slots' buffer, out_off); a, b and the guard slots
    are checked here."""
    import torch
    import fdeflate_amd as fd
    a, b = _uf_neighbours()
    want_a, want_b, empty = ob.compress_ultra_fast(a), ob.compress_ultra_fast(b), ob.compress_ultra_fast(b"")
    caps = [len(want_a), len(empty) + 3, big_cap, len(empty) + 3, len(want_b) + 7]
    out_off = np.zeros(6, dtype=np.int64)
    out_off[1:] = np.cumsum(caps)
    d_out = torch.full((int(out_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
    ln = fd.deflate_ultrafast_batch(d_in, torch.from_numpy(in_off).cuda(), d_out, torch.from_numpy(out_off).cuda())
    torch.cuda.synchronize()
    ln = ln.cpu().numpy().view(np.uint32)
    h = d_out.cpu().numpy()
    assert not harness.encoder_guard_faults(h, out_off, ln, empty, 0x5A)
    for i, w in ((0, want_a), (4, want_b)):
        assert int(ln[i]) == len(w) and h[out_off[i]:out_off[i] + len(w)].tobytes() == w, ("neighbour", i)
        assert np.all(h[out_off[i] + len(w):out_off[i + 1]] == 0x5A), ("neighbour", i)
    return ln, h, out_off


@pytest.mark.parametrize("n", [(1 << 31) + 13, (1 << 32) - 3])
def test_ultrafast_encoder_two_to_four_gib(harness, n):
    """The ultra-fast encoder between 2 and 4 GiB, where chunk numbers and Adler weights use the top bit of 32: zeros
    with a literal every 4099th byte, and the same with 0xFF in the last MiB (the Adler weights' worst case at the
    largest len), generated on the device, equal the oracle's encoder bit for bit (in a slot of the compressed length
    + 5, between two ordinary buffers) and decode back on the GPU to the buffer, its length and its Adler-32.  (The
    decode of 2^32 - 3 bytes is what met flush_ring's 32-bit line position coming round at 2^32: DESIGN.md "Size gates".)"""
    _need(3 * n + (3 << 30), "a %d-byte buffer, its decoded copy and the comparison" % n)
    for kind in ("sparse", "ff_tail"):
        def fill(v):
            v[::4099] = 1
            if kind == "ff_tail":
                v[-(1 << 20):] = 0xFF
        d_in, in_off, view = _uf_batch_around(n, fill)
        host = view.cpu().numpy()
        t0 = time.time()
        want = ob.compress_ultra_fast(host)
        t1 = time.time()
        ln, h, out_off = _uf_encode_around(harness, d_in, in_off, len(want) + 5)
        print("%s %d: oracle %.1f s, %d compressed bytes" % (kind, n, t1 - t0, len(want)))
        assert int(ln[2]) == len(want), (kind, int(ln[2]), len(want))
        assert h[out_off[2]:out_off[2] + len(want)].tobytes() == want, kind
        assert np.all(h[out_off[2] + len(want):out_off[3]] == 0x5A), kind
        del d_in, view
        st, dl, ad, slots, guards_ok = harness.gpu_inflate_big([want], [n])
        assert guards_ok and int(st[0]) == 0 and int(dl[0]) == n and int(ad[0]) == zlib.adler32(host), (kind, hex(int(st[0])), int(dl[0]))
        assert slots.head_equals(0, host), kind
        del slots


def test_ultrafast_encoder_input_of_four_gib_and_more(harness):
    """The ultra-fast encoder takes `len < 2^32` (the length comes back in 32 bits): device buffers of 2^32 and of
    2^32 + 1 zero bytes give out_len = 0xFFFFFFFF, nothing outside the slot changes, the neighbours are bit-exact.
    (2^32 - 3 bytes, the other side of the gate: test_ultrafast_encoder_two_to_four_gib.)"""
    _need(6 << 30, "a 4 GiB input")
    for n in (1 << 32, (1 << 32) + 1):
        d_in, in_off, view = _uf_batch_around(n, lambda v: None)
        ln, h, out_off = _uf_encode_around(harness, d_in, in_off, 1 << 20)
        assert int(ln[2]) == 0xFFFFFFFF, (n, int(ln[2]))
        del d_in, view
