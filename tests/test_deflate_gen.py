"""The foreign-stream corpus (tests/deflate_gen.py) on the CPU: every stream is valid for its writer, for zlib and for
the oracle alike, the corpus holds the edges it was built for, and its bytes are pinned -- so the GPU tests
(tests/test_gpu_foreign_streams.py) decode exactly what was checked here."""
import os
import re
import zlib

import numpy as np
import pytest

import deflate_gen as g
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SHA-256 over the streams of every class, in corpus order (deflate_gen.class_digests)
DIGESTS = {
    "U_nonzero_run": "c453c75a6913d650d662ad0b472385a2a0b93cf9eed0132161d416a3fe5b0043",
    "U_lanes_without_literals": "92d8551fe05e1a31b7345b1ee8cf7c4649a7f12da9bf09ce2a0f7e2ca39ce150",
    "U_offgrammar_zero": "74f6fa5af8850d53fa60923492d885bf7dbdf415bb542db9cfdb755e7bb47d83",
    "U_all_symbols": "918731d6813f32a3518cada19684f0c9d57b586dd93523a023c1a48846f6a3bd",
    "G_overlap_grid": "a0b7c6a8b41dd3580b5b88a36c7f74c25c9fd776ed71692ce90d5d547a62be3d",
    "G_ring_edges": "a3db3ec765d2ce12b1aa550f79adc8ae7e07f32523413310c6f507dd84f20a16",
    "G_window_start": "637d7b6fddb956b1663c366e4bda39c92c7f903b97f22769eb43b05a68780c61",
    "G_dense_matches": "fdb43c46d2c78f5b2ff35674792bd084bba9bc896849eaa8a58b3c772c45ece1",
    "G_expansion": "7c300729be028fdcf7fa5372b72562aada2c5a397e433d0cd307095cb083033f",
    "G_long_tokens": "738f58f9f611b6b4763d3da2cceb7745c6cca0e042634a7314d6e5a90351657e",
    "G_table_classes": "97303d7e03d3e2195d2c6b1981cda4403cc9412d43cb4a5afc060aeaf08bfaad",
    "G_headers": "732271290b637b3f3b518420b02fcff9a35397a236d8b4cc9f28d2401108ba63",
    "G_block_mix": "3fd1ddf1cd2b72756c12e2f8bd761106b977ac27e93026bf0e2d612a91270666",
    "errors": "daf00ce99e4adf424cc88ed2ce419a6060dc0a5bfc1cf286f1639ad45ec396e0",
    "truncations": "72daa34d6501992bd32a150d1dc473cdb5222126125160f696abde53a34ba526",
}


def _lz_constants():
    """FDH_LZ_LIT_BITS, FDH_LZ_DIST_BITS, FDH_LZ_SUB, FDH_LZ_DSUB as inflate_lz.h defines them"""
    with open(os.path.join(ROOT, "fdeflate_amd", "csrc", "inflate_lz.h")) as f:
        text = f.read()
    out = {}
    for key, name in (("lit_bits", "FDH_LZ_LIT_BITS"), ("dist_bits", "FDH_LZ_DIST_BITS"), ("sub", "FDH_LZ_SUB"),
                      ("dsub", "FDH_LZ_DSUB")):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
        assert m, "%s not found in inflate_lz.h" % name
        out[key] = int(m.group(1))
    return out


def test_bit_writer_and_codes_against_the_quadratic_writer():
    """The byte-flushing writer, its vectorised path included, writes what streams.BitWriter writes."""
    import streams
    r = np.random.default_rng(1)
    a, b = g.BitWriter(), streams.BitWriter()
    for _ in range(300):
        n = int(r.integers(1, 49))
        v = int(r.integers(0, 1 << n))
        a.bits(v, n)
        b.bits(v, n)
        if r.random() < 0.1:
            lens = r.integers(1, 16, int(r.integers(1, 40)))
            codes = np.array([int(r.integers(0, 1 << int(l))) for l in lens])
            a.many(codes, lens)
            for c, l in zip(codes.tolist(), lens.tolist()):
                b.bits(c, l)
        if r.random() < 0.05:
            data = bytes(r.integers(0, 256, 5, dtype=np.uint8))
            a.raw(data)
            b.raw(data)
        assert a.bitpos() == b.n
    assert a.tobytes() == b.tobytes()
    lens = streams.long_code_lengths()
    ref = streams.canonical_codes(lens)
    mine = g.canonical_codes(lens)
    assert all(mine[s] == ref[s] for s in ref) and sum(1 for c in mine if c) == len(ref)


def test_ultrafast_prefix_is_the_encoders():
    head, low = g.uf_prefix()
    empty = ob.compress_ultra_fast(b"")
    assert head == empty[:53] and low == empty[53] & 31
    assert g.uf_foreign([])[0] == empty


def _encoder_inputs():
    """the inputs of test_ultrafast_encode_bit_exact (tests/test_gpu_parity.py) up to 70 001 bytes"""
    from fdeflate_amd import synth
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
    for i in (0, 1, 7, 15, 16, 23):
        raws.append(synth.gen_stream_np(i, 65536).tobytes())
    return raws


def test_reference_policy_is_the_encoder_byte_for_byte():
    """uf_parse(raw, "reference") through uf_foreign is ob.compress_ultra_fast(raw): that pins the writer -- prefix,
    code, token layout, trailer -- to the one encoder whose streams the kernels were written around."""
    for i, raw in enumerate(_encoder_inputs()):
        comp, payload = g.uf_foreign(g.uf_parse(raw, "reference"))
        assert payload == raw, i
        assert comp == ob.compress_ultra_fast(raw), (i, len(raw))


def test_every_policy_spells_the_same_payload():
    r = np.random.default_rng(5)
    x = r.integers(0, 256, 30000, dtype=np.uint8)
    x[r.random(x.size) < 0.5] = 0
    x[100:900] = 0
    x[5000:9000] = 0xFF
    x[20000:20007] = 3
    seen = set()
    for pol in g.UF_POLICIES:
        toks = g.uf_parse(x, pol, seed=3, long258=True)
        comp, payload = g.uf_foreign(toks)
        assert payload == x.tobytes() and zlib.decompress(comp) == payload, pol
        st = g.token_stats(toks)
        seen.add(comp)
        if pol == "literals_only":
            assert st["matches"] == 0
        if pol == "threes":
            assert st["lengths"] == {3}
        if pol == "fours":
            assert st["lengths"] == {4}
        if pol == "random_cuts":
            big = g.uf_parse(bytes(300000), pol, seed=1)
            lengths = g.token_stats(big)["lengths"]
            assert {g._LEN_SYM[l] for l in lengths} == set(range(29))           # every length symbol
            for i in range(29):                                                   # ... at its lowest and highest extra value
                assert g.LEN_BASE[i] in lengths and min(g.LEN_BASE[i] + (1 << g.LEN_EXTRA[i]) - 1, 258) in lengths, i
    assert len(seen) == len(g.UF_POLICIES)      # one payload, seven streams


def test_three_way_agreement():
    """Every stream of the corpus decodes to the writer's own payload by zlib and by the oracle (status Ok, matching
    Adler-32), in a slot of exactly the payload's size.  The share on which the three disagree is zero."""
    rows = g.corpus()
    assert sum(len(x[3]) for x in rows) <= g.MAX_PAYLOAD and {x[0] for x in rows} == set(g.CLASSES)
    bad = []
    for cls, name, comp, raw in rows:
        try:
            z = zlib.decompress(comp)
        except zlib.error as ex:
            z = ex
        st, out, ad = ob.decompress_bounded(comp, len(raw))
        if not (z == raw and st == 0 and out == raw and ad == zlib.adler32(raw)):
            bad.append((cls, name, z if isinstance(z, Exception) else len(z), ob.STATUS_NAMES[st], len(out), len(raw)))
    assert not bad, (len(bad), bad[:8])
    core = g.core()
    assert sum(len(x[3]) for x in core) <= g.MAX_CORE and {x[0] for x in core} == set(g.CLASSES)


def test_error_corpus_statuses():
    named = 0
    for cls, name, comp, exp in g.error_corpus():
        st, _, _ = ob.decompress_bounded(comp, 1 << 16)
        assert st != 0, (cls, name)
        with pytest.raises(zlib.error):
            zlib.decompress(comp)
        if exp is not None:
            named += 1
            assert ob.STATUS_NAMES[st] == exp, (cls, name, ob.STATUS_NAMES[st], exp)
    names = [x[1] for x in g.error_corpus()]
    assert named >= 13 and "run_first" in names and "distance_bit_set" in names
    assert sum(1 for n in names if "_cut" in n) == 6


def test_classify_code():
    """The classifier on codes whose class is known by construction."""
    flat = [8] * 226 + [9] * 60
    assert g.classify_code(flat, 9, 256) == ("none", dict(prefixes=0, entries=0, fitted=0))
    assert g.classify_code(flat, 8, 256)[0] == "second_level"
    assert g.classify_code(flat, 8, 256)[1] == dict(prefixes=30, entries=60, fitted=30)
    assert g.classify_code(flat, 8, 59)[0] == "overflow" and g.classify_code(flat, 8, 59)[1]["fitted"] == 29
    assert g.classify_code(flat, 8, 1)[0] == "walk_only"
    # streams.valid_streams' dyn_longdist: one prefix that asks for 128 entries
    dl = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]
    assert g.classify_code(dl, 8, 64) == ("walk_only", dict(prefixes=1, entries=128, fitted=0))
    assert g.classify_code(dl, 8, 128)[0] == "second_level"
    # the offset runs on over a prefix that did not fit: a small one behind a big one does not fit either
    # the offset runs on over a prefix that did not fit: whichever of these two comes first, the other does not fit
    two = g.shaped_code(30, 8, g.chain(8, 14) * 2, np.random.default_rng(1))
    assert g.classify_code(two, 8, 64) == ("overflow", dict(prefixes=2, entries=66, fitted=1))


def test_corpus_holds_its_edges():
    rows, info = g.corpus(), g.corpus_info()
    by = {}
    for cls, name, comp, raw in rows:
        by.setdefault(cls, []).append((name, comp, raw, info[(cls, name)]))
    k = _lz_constants()
    assert k == g.LZ_CONSTANTS, "deflate_gen.LZ_CONSTANTS no longer matches inflate_lz.h: rebuild the corpus and its digests"

    # ---- the table classes, under the header's constants ----
    codes = g.table_class_codes(**k)
    for which, bits, cap in (("lit", k["lit_bits"], k["sub"]), ("dist", k["dist_bits"], k["dsub"])):
        for cls in g.TABLE_CLASSES:
            # one prefix asks for at most 2^(15 - bits) entries: with `cap` at or above that the first prefix in
            # ascending order always fits, and no code is walk_only (the literal/length table at 9 bits / 256 entries)
            exists = not (cls == "walk_only" and (1 << (15 - bits)) <= cap)
            assert ((which, cls) in codes) == exists, (which, cls)
            if exists:
                assert g.classify_code(codes[(which, cls)], bits, cap)[0] == cls, (which, cls)
                assert any(n == "%s_%s" % (which, cls) for n, _, _, _ in by["G_table_classes"])
    assert len(codes) >= 7
    for (which, cls), lens in codes.items():      # every symbol of the code has a code: the blocks use each of them
        assert all(lens), (which, cls)

    # ---- every (len, dist <= len) ----
    pairs = set()
    for name, comp, raw, inf in by["G_overlap_grid"]:
        if name.endswith("_fixed"):
            pairs.update(inf["matches"])
        else:
            twin = next(x for x in by["G_overlap_grid"] if x[0] == name.replace("_dyn", "_fixed"))
            assert twin[2] == raw and twin[3]["matches"] == inf["matches"]
    assert pairs == {(ln, d) for ln in range(3, 259) for d in range(1, ln + 1)} and len(pairs) == 33408

    # ---- ring edges: every pair in all 64 streams, whose payloads differ by the literals in front ----
    want = {(ln, d) for ln in g.RING_LENS for d in (ln, ln + 1) + g.RING_DISTS}
    sizes = set()
    for name, comp, raw, inf in by["G_ring_edges"]:
        assert want <= set(inf["matches"]), name
        sizes.add(len(raw) % 64)
    assert len(by["G_ring_edges"]) == 64 and sizes == set(range(64))

    # ---- stored headers at all eight bit phases, with and without payload ----
    for name, comp, raw, inf in by["G_block_mix"]:
        if name.startswith("mix300"):
            assert {p for p, n in inf["stored_phases"]} == set(range(8)), name
            assert {p for p, n in inf["stored_phases"] if n} == set(range(8)), name
    # ... and a match that reaches back over the stored bytes of another block
    name, comp, raw, inf = next(x for x in by["G_block_mix"] if x[0] == "stored65535")
    assert all(30000 <= d <= 32768 for _, d in inf["matches"]) and len(inf["matches"]) == 600

    # ---- every repeat count ----
    seen = set()
    for name, comp, raw, inf in by["G_headers"]:
        seen.update((s, e) for s, e in inf["cl_syms"] if s >= 16)
    assert seen >= ({(16, e) for e in range(4)} | {(17, e) for e in range(8)} | {(18, e) for e in range(128)})
    assert {n for n, _, _, _ in by["G_headers"]} >= {"hclen%d" % h for h in range(5, 20)}

    # ---- dense matches: more per 4096 stream bits than a tile's list, more per image than the image's list ----
    dense = 0
    for name, comp, raw, inf in by["G_dense_matches"]:
        first, end = inf["block_bits"][0]
        m = len(inf["matches"])
        if m * 4096 > 192 * (end - first) and m * 3328 > 832 * len(raw):
            dense += 1
    assert dense == len(by["G_dense_matches"]) == 5

    # ---- several lanes' ranges of run tokens only ----
    assert any(64 * inf["chain_bits"] > 3 * inf["data_bits"] for _, _, _, inf in by["U_lanes_without_literals"])
    assert all(len(comp) >= 8192 for _, comp, _, _ in by["U_lanes_without_literals"])

    # ---- 48-bit tokens ----
    name, comp, raw, inf = next(x for x in by["G_long_tokens"] if x[0] == "tok48")
    first, end = inf["block_bits"][0]
    assert len(inf["matches"]) == 500 and end - first >= 500 * 48 + 32768 * 8


def test_truncations_shape():
    t = g.truncations()
    assert len({n.split("/")[0] for n, _ in t}) == len(g.CLASSES)
    assert all(30 <= sum(1 for n, _ in t if n.startswith(cls + "/")) <= 36 for cls in g.CLASSES)


def test_corpus_digests():
    """One SHA-256 per class: the streams decoded on the GPU box are, provably, the bytes checked here."""
    assert g.class_digests() == DIGESTS
