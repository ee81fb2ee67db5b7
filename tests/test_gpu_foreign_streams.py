"""-m gpu: valid streams that neither zlib nor this project's encoders write (tests/deflate_gen.py; checked on the CPU
by tests/test_deflate_gen.py, which pins their bytes) through the whole pipeline, through every decoder variant and
through each kernel on its own, against the oracle -- bit-exact."""
import zlib

import numpy as np
import pytest

import deflate_gen as g
import oracle_binding as ob

pytestmark = pytest.mark.gpu

PENDING = 0xFFFFFFFD      # status at or above: left to the kernels that did not run


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


def _slots(rows):
    names, blobs, caps = [], [], []
    for cls, name, comp, raw in rows:
        for c in g.caps_for(len(raw)):
            names.append("%s/%s@%d" % (cls, name, c))
            blobs.append(comp)
            caps.append(c)
    return names, blobs, caps


@pytest.mark.parametrize("cls", g.CLASSES)
def test_whole_pipeline(harness, cls):
    """Every stream of a class in exact, loose, short, half and empty slots, with and without the checksum."""
    names, blobs, caps = _slots([x for x in g.corpus() if x[0] == cls])
    for flags in (0, 1):
        harness.assert_inflate_parity(names, blobs, caps, flags=flags)


def test_error_corpus(harness):
    rows = g.error_corpus()
    names, blobs, caps = [], [], []
    for cls, name, comp, exp in rows:
        for c in (65536, 4, 0):
            names.append("%s/%s@%d" % (cls, name, c))
            blobs.append(comp)
            caps.append(c)
    for flags in (0, 1):
        harness.assert_inflate_parity(names, blobs, caps, flags=flags)
    st = harness.gpu_inflate(blobs, caps)[0]
    for k, (cls, name, comp, exp) in enumerate(rows):     # in the large slot: the status the stream was made for
        if exp is not None:
            assert ob.STATUS_NAMES[int(st[3 * k])] == exp, (name, int(st[3 * k]), exp)


def test_truncations(harness):
    """One stream of every class cut at 24 seeded places and at its last 12 bytes: the oracle's status, and for
    InsufficientInput the length and the bytes its streaming `read` had produced when the input ran out."""
    import random
    items = g.truncations()
    names = [n for n, _ in items]
    blobs = [b for _, b in items]
    rnd = random.Random(3)
    for caps in ([1 << 17] * len(blobs), [rnd.choice((65536, 40000, 30000, 12345, 1000)) for _ in blobs]):
        partial = {}
        for i, blob in enumerate(blobs):
            d = ob.Decompressor()
            out = np.zeros(caps[i], dtype=np.uint8)
            st, c, p = d.read(blob, out, 0)
            if st == 0 and not d.is_done() and p < caps[i]:
                partial[i] = out[:p].tobytes()
        assert len(partial) > 100
        for flags in (0, 1, 0x1000):
            harness.assert_inflate_parity(names, blobs, caps, flags=flags)
            st, ln, ad, outs, ok = harness.gpu_inflate(blobs, caps, flags)
            for i, data in partial.items():
                assert int(st[i]) == 2, (names[i], int(st[i]), flags)
                assert int(ln[i]) == len(data) and outs[i][:len(data)].tobytes() == data, (names[i], int(ln[i]), len(data), flags)


# 256: span decoder (experimental); 0x400: without the interval kernel; 0x1000: without the LZ-window
# kernel (the tile decoders take the general streams, as before round 4); round 5: 0x10000 without the
# landing decoder, 0x80000 the landing decoder with the general writing pass only, 0x100000 one stream
VARIANTS = (8, 4 | 8, 2, 16, 16 | 8, 128, 128 | 8, 256, 256 | 8, 256 | 4 | 8, 0x400, 0x400 | 8, 0x1000, 0x1000 | 8,
            0x10000, 0x10000 | 8, 0x80000, 0x80000 | 8, 0x100000)


def _variant_rows():
    core = g.core()
    have = {(x[0], x[1]) for x in core}
    return core + [x for x in g.corpus() if x[0].startswith("U_") and (x[0], x[1]) not in have]


@pytest.mark.parametrize("flags", VARIANTS, ids=["%#x" % f for f in VARIANTS])
def test_every_decoder_variant(harness, flags):
    """The core subset and everything behind the ultra-fast prefix through each decoder on its own: with the
    re-check off a tile-decoder bug cannot hide behind the exact serial path."""
    names, blobs, caps = [], [], []
    for cls, name, comp, raw in _variant_rows():
        for c in (len(raw), len(raw) + 100):
            names.append("%s/%s@%d" % (cls, name, c))
            blobs.append(comp)
            caps.append(c)
    harness.assert_inflate_parity(names, blobs, caps, flags=flags)


# ---- each kernel alone ----
LANDING, LANDING_GENERAL, INTERVALS, SEGMENTS, BOTH, LZ = 0x20000, 0x20000 | 0x80000, 0x800, 0x400 | 64, 64, 0x2000
U_CLASSES = tuple(c for c in g.CLASSES if c.startswith("U_"))
G_CLASSES = tuple(c for c in g.CLASSES if c.startswith("G_"))
TAKES_ALL, MAY_PASS_ON = "takes all", "may pass on"


def _group(cls, name):
    """The unit of the expectation table: a class, split by how its run tokens are cut where that decides."""
    if cls == "U_offgrammar_zero":
        return cls + ":" + next((p for p in g.OFFGRAMMAR_POLICIES if name.endswith("_" + p)), name)
    if cls == "U_lanes_without_literals":
        return cls + (":fours" if name.endswith("_fours") else ":any_byte")
    return cls


# Why a kernel may leave a valid stream to the kernels behind it (that costs speed only: test_whole_pipeline decides
# correctness).  Each reason names the code that passes the stream on.
_LEAN = ("the lean writer leaves its zero-initialised image alone for a run chain and sends a chain behind a non-zero byte on: "
         "front != 0 || wq + xi == 0, inflate_seg3.h:728-736, :830-832 (slots at a multiple of 16 only: :161)")
_SLOTS3 = ("a run token that is not 258 bytes long ends its chain (inflate_seg3.h:367), every chain ends an interval and takes one "
           "of the lane's kS2Slots = 48 check-point slots (:396, :315-323; inflate_seg2.h:57); a lane with more such tokens "
           "in its range faults (:318) and the stream is passed on (:502, :528-530)")
_SLOTS2 = ("a run token that is not 258 bytes long ends its chain (inflate_seg2.h:327), every chain ends an interval and takes one "
           "of the lane's kS2Slots = 48 check-point slots (:332-337, :57); out of slots: left to the other kernels (:271, :335-336)")
_PERIODIC3 = ("thousands of equal literals in a row: guessed chains inside a periodic stretch need not fall in step with the real "
              "one, and lanes that have not landed after four rounds pass the stream on (inflate_seg3.h:401, :484, :502)")
_PERIODIC2 = "as above with six rounds: giveup, inflate_seg2.h:553-560, :612"
_PERIODIC1 = "as above with six rounds: giveup, inflate_segments.h:803-811, :861"
_BREAKS = ("supposed, from the code alone: a round of 64 intervals that are all long run chains leaves kS2MaxBreaks = 64 breaks "
           "in the image, which the writer refuses (inflate_seg2.h:758-759, :1086); run200000 holds 97 chains of eight tokens; "
           "seen with 16-byte aligned slots only")
_STORED = "stored blocks: the kernel only takes Huffman blocks, bails at a stored one and hands over at a ResumePoint, inflate_lz.h:35-36"

EXPECT = {}   # (flags, group) -> (expectation, reason for a "may pass on": code, file and line)
_OFF = "U_offgrammar_zero:"
for _f, _why_slots, _why_periodic in ((LANDING, _SLOTS3, _PERIODIC3), (LANDING_GENERAL, _SLOTS3, _PERIODIC3), (INTERVALS, _SLOTS2, _PERIODIC2),
                              (BOTH, None, _PERIODIC2 + "; " + _PERIODIC1), (SEGMENTS, None, _PERIODIC1)):
    for _grp in ("U_nonzero_run", "U_lanes_without_literals:any_byte", "U_all_symbols", _OFF + "tail_first", _OFF + "chain258_broken"):
        EXPECT[(_f, _grp)] = (TAKES_ALL, "")
    for _grp in ("U_lanes_without_literals:fours", _OFF + "threes", _OFF + "fours", _OFF + "random_cuts", _OFF + "chain200_non258"):
        # the segment kernel decodes token by token and keeps no check points: it takes them, alone and behind the interval kernel
        EXPECT[(_f, _grp)] = (MAY_PASS_ON, _why_slots) if _why_slots else (TAKES_ALL, "")
    EXPECT[(_f, _OFF + "literals_only")] = (MAY_PASS_ON, _why_periodic)
for _grp in ("U_nonzero_run", "U_lanes_without_literals:any_byte"):
    EXPECT[(LANDING, _grp)] = (MAY_PASS_ON, _LEAN)
for _f in (LANDING_GENERAL, INTERVALS):
    EXPECT[(_f, "U_lanes_without_literals:any_byte")] = (MAY_PASS_ON, _BREAKS)
for _c in G_CLASSES:   # "any zlib stream of Huffman blocks", inflate_lz.h:1-2
    EXPECT[(LZ, _c)] = (TAKES_ALL, "") if _c != "G_block_mix" else (MAY_PASS_ON, _STORED)


def _alone(harness, flags, classes):
    """-> {(slots, group): [names left PENDING]}; slots "odd": exact slots at odd addresses (guards of 5 bytes), "loose":
    16 bytes more, "aligned": every slot at a multiple of 16 and up to 15 bytes loose -- the only slots the landing
    decoder's lean writer takes (inflate_seg3.h:161).  Whatever is reported is checked."""
    rows = [x for x in g.corpus() if x[0] in classes]
    blobs = [x[2] for x in rows]
    left = {}
    for slots in ("odd", "loose", "aligned"):
        caps = [len(x[3]) + 16 if slots == "loose" else (len(x[3]) + 15) & ~15 if slots == "aligned" else len(x[3]) for x in rows]
        st, ln, ad, outs, guards_ok = harness.gpu_inflate(blobs, caps, flags=flags, guard=16 if slots == "aligned" else 5)
        assert guards_ok, "a kernel wrote outside its slot (flags %#x)" % flags
        for i, (cls, name, comp, raw) in enumerate(rows):
            if int(st[i]) >= PENDING:
                left.setdefault((slots, _group(cls, name)), []).append(name)
                continue
            # whatever is reported is the oracle's answer; these streams are valid, so that is Ok and the payload
            assert int(st[i]) == 0, (cls, name, int(st[i]), flags, slots)
            assert int(ln[i]) == len(raw) and outs[i][:len(raw)].tobytes() == raw, (cls, name, flags, slots)
            assert int(ad[i]) == zlib.adler32(raw), (cls, name, flags, slots)
    total = {}
    for cls, name, _, _ in rows:
        total[_group(cls, name)] = total.get(_group(cls, name), 0) + 1
    for (slots, grp), names in sorted(left.items()):
        print("flags %#x %s %s: left %d of %d, e.g. %s" % (flags, slots, grp, len(names), total[grp], names[:3]))
    return left, total


def _check_expectations(flags, left, total):
    for grp in total:
        what, why = EXPECT[(flags, grp)]
        assert what in (TAKES_ALL, MAY_PASS_ON) and (what == TAKES_ALL or len(why) > 20), (hex(flags), grp)
        if what == TAKES_ALL:
            gone = {s: v for (s, g_), v in left.items() if g_ == grp}
            assert not gone, (hex(flags), grp, {s: (len(v), v[:5]) for s, v in gone.items()})


@pytest.mark.parametrize("flags", (LANDING, LANDING_GENERAL, INTERVALS, SEGMENTS, BOTH), ids=lambda f: "%#x" % f)
def test_each_prefix_kernel_alone(harness, flags):
    """The landing decoder (lean and general writing pass), the interval kernel, the segment kernel and the two
    together on everything behind the ultra-fast prefix: a stream may be left PENDING; whatever is reported is the
    oracle's status, length, bytes and Adler-32, and the guard slots are intact.  What must not be left: EXPECT."""
    left, total = _alone(harness, flags, U_CLASSES)
    _check_expectations(flags, left, total)


@pytest.mark.parametrize("cls", G_CLASSES)
def test_lz_window_kernel_alone(harness, cls):
    """FDH_FLAG_LZ_ONLY on the general classes: it takes every stream of Huffman blocks (inflate_lz.h:1-2)."""
    left, total = _alone(harness, LZ, (cls,))
    _check_expectations(LZ, left, total)


@pytest.mark.parametrize("cls", g.CLASSES)
def test_whole_pipeline_aligned_slots(harness, cls):
    """The whole pipeline once more with every slot at a multiple of 16 bytes: gpu_harness packs slots at odd
    addresses, where the landing decoder's lean writer never runs (inflate_seg3.h:161)."""
    rows = [x for x in g.corpus() if x[0] == cls]
    caps = [(len(x[3]) + 15) & ~15 for x in rows]
    for flags in (0, 0x10000):
        st, ln, ad, outs, guards_ok = harness.gpu_inflate([x[2] for x in rows], caps, flags=flags, guard=16)
        assert guards_ok
        for i, (_, name, comp, raw) in enumerate(rows):
            assert int(st[i]) == 0 and int(ln[i]) == len(raw), (cls, name, int(st[i]), int(ln[i]), flags)
            assert outs[i][:len(raw)].tobytes() == raw and int(ad[i]) == zlib.adler32(raw), (cls, name, flags)


def test_fused_png_decode(harness):
    """fd.inflate_png_batch on 64 images of 32 rows x 97 bytes, bpp 3, whose filtered rows -- flat stretches of every
    byte value, every filter type -- are written with run tokens behind non-zero bytes and with random cuts."""
    import torch
    import fdeflate_amd as fd
    import streams
    r = np.random.default_rng(41)
    n, rows, rb, bpp = 64, 32, 97, 3
    filts, comps = [], []
    for i in range(n):
        f = r.integers(0, 256, (rows, rb + 1), dtype=np.uint8)
        f[:, 0] = r.integers(0, 5, rows)
        for _ in range(12):                      # flat stretches inside a row and over several rows
            a = int(r.integers(0, f.size - 8))
            f.reshape(-1)[a:a + int(r.integers(6, 400))] = int(r.integers(0, 256)) if r.random() < 0.8 else 0
        f[:, 0] %= 5
        filts.append(f.tobytes())
        toks = g.uf_parse(filts[-1], "any_byte" if i % 2 == 0 else "random_cuts", seed=i, long258=True)
        assert any(isinstance(t, tuple) for t in toks)
        comp, payload = g.uf_foreign(toks)
        assert payload == filts[-1]
        comps.append(comp)
    cbuf, coff = streams.pack_exact(comps)
    foff = np.arange(n + 1, dtype=np.int64) * (rows * (rb + 1))
    poff = np.arange(n + 1, dtype=np.int64) * (rows * rb)
    d_f = torch.zeros(int(foff[-1]), dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(int(poff[-1]), dtype=torch.uint8, device="cuda")
    out_len, status, adler, pst = fd.inflate_png_batch(torch.from_numpy(cbuf).cuda(), torch.from_numpy(coff.astype(np.int64)).cuda(),
                                                       d_f, torch.from_numpy(foff).cuda(), d_p, torch.from_numpy(poff).cuda(), rb, bpp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n and pst.cpu().tolist() == [0] * n
    assert out_len.cpu().tolist() == [rows * (rb + 1)] * n
    hp, hf, ad = d_p.cpu().numpy(), d_f.cpu().numpy(), adler.cpu().numpy().view(np.uint32)
    for i in range(n):
        est, epix = ob.png_unfilter(filts[i], rb, bpp)
        assert est == 0
        assert hf[foff[i]:foff[i + 1]].tobytes() == filts[i], i
        assert hp[poff[i]:poff[i + 1]].tobytes() == epix, i
        assert int(ad[i]) == zlib.adler32(filts[i]), i


def _resumable_cases():
    """-> list of (name, stream, payload, a cut of the input that must be among the cuts)"""
    r = np.random.default_rng(43)
    out = []
    for k, (run, v) in enumerate(((258 * 64 + 2, 0x80), (5000, 1), (258 * 6 + 1, 0xFF), (30000, 0x41))):
        x = r.integers(0, 256, 20000 + run, dtype=np.uint8)
        x[r.random(x.size) < 0.3] = 0
        x[9000:9000 + run] = v
        x[8999] = v ^ 0x55
        toks = g.uf_parse(x, "any_byte" if k % 2 == 0 else "random_cuts", seed=k)
        first = next(i for i, t in enumerate(toks) if isinstance(t, tuple) and sum(isinstance(u, tuple) for u in toks[i:i + 4]) == 4)
        chain = next(j for j in range(len(toks) - first + 1) if first + j == len(toks) or not isinstance(toks[first + j], tuple))
        inside = len(g.uf_foreign(toks[:first + chain // 2], end=False)[0])      # a cut inside the run chain
        comp, raw = g.uf_foreign(toks)
        out.append(("U_run%d" % run, comp, raw, inside))
    lit_l = g.spread(g.complete_code(286, 11, r, deep=0.1), list(range(286)), r, 286)
    dist_l = g.spread(g.complete_code(30, 7, r, deep=0.1), list(range(30)), r, 30)
    for k, nstored in enumerate((20000, 65535)):
        sw = g.StreamWriter()
        sw.dynamic([bytes(r.integers(0, 256, 9000, dtype=np.uint8))], lit_l, dist_l, r=r)
        inside = len(sw.w.tobytes()) + 5 + nstored // 2                      # a cut inside the stored block
        sw.stored(bytes(r.integers(0, 256, nstored, dtype=np.uint8)))
        toks = []
        for _ in range(300):
            toks += [g.M(int(r.integers(3, 259)), int(r.integers(1, min(nstored + 9000, 32768)))), bytes(r.integers(0, 256, 2, dtype=np.uint8))]
        sw.fixed(toks, final=True)
        comp, raw = sw.finish()
        out.append(("G_stored%d" % nstored, comp, raw, inside))
    for name in ("phase07", "phase32"):
        cls, _, comp, raw = next(x for x in g.corpus() if x[0] == "G_ring_edges" and x[1] == name)
        out.append(("G_ring_" + name, comp, raw, len(comp) - 3000))          # far into the matches behind the literals
    return out


def test_resumable_decode(harness):
    """fdh_inflate_batch_resumable, every call checked on its own (gpu_harness.drive_resumable, per_call): four
    streams with run chains behind a non-zero byte, four general ones (stored blocks between Huffman blocks, ring
    edges); three cuts of the input, one of them inside a run chain / a stored block, and two of the slot."""
    import fdeflate_amd as fd
    cases = _resumable_cases()
    comps = [c[1] for c in cases]
    in_cuts, out_cuts = [], []
    for name, comp, raw, inside in cases:
        assert 60 < inside < len(comp) - 8, (name, inside, len(comp))
        in_cuts.append(sorted({len(comp) // 5, inside, len(comp) - 2}) + [len(comp)])
        out_cuts.append([len(raw) // 2, len(raw) - 1, len(raw)])
        assert len(in_cuts[-1]) == 4
    res, outs, guards, _ = harness.drive_resumable(fd, comps, in_cuts, out_cuts, per_call=True)
    assert guards
    ln, st, ad = res
    for i, (name, comp, raw, _) in enumerate(cases):
        assert int(st[i]) == 0 and int(ln[i]) == len(raw) and outs[i][:len(raw)].tobytes() == raw, (name, int(st[i]), int(ln[i]))
        assert int(ad[i]) == zlib.adler32(raw), name
