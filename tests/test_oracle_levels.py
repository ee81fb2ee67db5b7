"""CPU checks of the oracle's encoders of levels 2..9 (oracle/fdeflate_oracle.c: HashChainMatchFinder, HybridMatchFinder,
LazyParser::compress, restated in C from the Rust) against the two pure-Python models (tests/level_model.py,
tests/lazy_model.py), which are another reading of the same Rust.

- bytes: ob.compress_level equals level_model at levels 2 and 3 and lazy_model at 4, 5, 6 and 9 over every shared input;
  7 and 8 equal 9; level 1 equals compress_level1, level 0 compress_stored, 10 and above 7;
- branches: the oracle's coverage counters summed over those inputs equal the model's, counter by counter, so the two agree
  on which way every step went and not only on the bytes;
- the eight long low-entropy inputs that the model's time keeps out of levels 5, 6 and 9 go through the oracle there;
- every oracle stream round-trips through zlib and through the oracle's own decoder and fits the bound;
- the volume corpus (streams.level_volume_inputs, 2 000 streams, 10.3 MB) meets at every level 2..9, with the oracle
  alone, everything tests/test_gpu_levels_oracle.py requires of it (level_volume.unmet_requirements).

Oracle wall time over the volume corpus, 16 threads, one batch per level (measured on the build machine, 2026-10):
level 2 0.14 s, 3 0.15 s, 4 0.25 s, 5 0.30 s, 6 0.28 s, 7 / 8 / 9 0.07 s each -- the critical path is the longest
stream, not the sum.  The model needs about 100 s for the shared inputs of the six levels; the oracle 1.5 s.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import lazy_model as zm
import level_model as lm
import level_volume as lv
import oracle_binding as ob
import streams

LAZY = (4, 5, 6, 9)
EMPTY = bytes.fromhex("7801030000000001")


def _both_decoders(out, x, what):
    assert out[:2] == b"\x78\x01", what
    assert zlib.decompress(out) == x, what
    st, back, _ = ob.decompress_bounded(out, len(x))
    assert st == 0 and back == x, (what, st)
    assert len(out) <= lv.compress_bound(len(x)), (what, len(out))


def _rows(level):
    return lm.model_results()[level] if level in (2, 3) else zm.model_results()[level]


@pytest.fixture(scope="module")
def oracle_rows():
    """level -> (streams, counters) of the oracle over the model's shared inputs of that level"""
    res = {}
    for level in (2, 3) + LAZY:
        ob.level_counters_reset()
        outs = [ob.compress_level(x, level) for x, _, _ in _rows(level)]
        res[level] = (outs, ob.level_counters(reset=True))
    return res


@pytest.mark.parametrize("level", (2, 3) + LAZY)
def test_oracle_equals_the_model_on_every_shared_input(oracle_rows, level):
    outs, _ = oracle_rows[level]
    rows = _rows(level)
    bad = [(i, len(x), len(o), len(w)) for i, ((x, w, _), o) in enumerate(zip(rows, outs)) if o != w]
    assert not bad, (level, len(bad), bad[:8])
    for i, ((x, _, _), o) in enumerate(zip(rows, outs)):
        _both_decoders(o, x, (level, i, len(x)))


@pytest.mark.parametrize("level", (2, 3) + LAZY)
def test_oracle_counters_equal_the_models(oracle_rows, level):
    """Summed over the shared inputs (maxima where the name says so).  At levels 2 and 3 the model counts the finder's
    exits only.  `unwritten` is the model's alone (the oracle clears its ring, as the Rust does)."""
    _, got = oracle_rows[level]
    want = {}
    for _, _, c in _rows(level):
        zm.add_counters(want, c)
    want.pop("unwritten")
    assert set(want) <= set(ob.LEVEL_COUNTERS)
    if level >= 4:
        assert set(want) == set(zm.FINDER_COUNTERS + zm.LOOP_COUNTERS) - {"unwritten"}
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    print("level %d oracle counters: %r" % (level, got))
    assert not diff, (level, diff)


def test_levels_7_8_and_above_are_level_9_and_levels_0_and_1_are_the_calls_that_were_there():
    rows = zm.model_results()[9]
    for level in (7, 8, 10, 255):
        bad = [i for i, (x, w, _) in enumerate(rows) if ob.compress_level(x, level) != w]
        assert not bad, (level, bad[:8])
    for x in streams.encoder_inputs():
        assert ob.compress_level(x, 1) == ob.compress_level1(x), len(x)
        assert ob.compress_level(x, 0) == ob.compress_stored(x), len(x)
    for level in range(1, 12):
        assert ob.compress_level(b"", level) == EMPTY, level


def test_small_slots_are_refused_not_overrun():
    x = np.frombuffer(streams.chain_inputs()[8][:20000], dtype=np.uint8)
    for level in range(10):
        full = ob.compress_level(x, level)
        for cap in (0, 1, len(full) // 2, len(full) - 1):
            out = np.full(cap + 64, 0x5A, dtype=np.uint8)
            n = ob.lib().fdo_compress_level(x.ctypes.data_as(C.c_void_p), x.size, level, out.ctypes.data_as(C.c_void_p), cap)
            assert n == 0 and np.all(out[cap:] == 0x5A), (level, cap, n)


@pytest.mark.parametrize("level", (5, 6, 9))
def test_the_long_low_entropy_inputs_the_model_leaves_out(level):
    """lazy_model.shared_inputs() drops eight of the nine long inputs over 3 or 4 symbols at levels 5, 6 and 9 (110 s of
    model time at level 6); the oracle takes them in well under a second.  Level 4, where the model keeps them, pins
    the oracle on exactly these inputs (test_oracle_equals_the_model_on_every_shared_input); here they round-trip and
    fit the bound at the deeper levels."""
    shared = zm.shared_inputs()
    left_out = [x for x in shared[4] if x not in set(shared[level])]
    assert len(left_out) == 8 and all(len(x) in (120000, 300000) and max(x) <= 3 for x in left_out)
    assert all(any(x == y for y, _, _ in zm.model_results()[4]) for x in left_out)
    ob.level_counters_reset()
    for i, x in enumerate(left_out):
        _both_decoders(ob.compress_level(x, level), x, (level, i, len(x)))
    c = ob.level_counters(reset=True)
    assert c["maxsteps"] == lv.DEPTH[level] and c["alias"] > 0 and c["blocks"] > 0 and c["pass2_base"] > 32768, c


def test_volume_corpus_is_what_it_says():
    rows, info = streams.level_volume_inputs()
    streams._volume_cache.clear()       # drawn again from the fixed seeds: the same bytes
    again, _ = streams.level_volume_inputs()
    assert again == rows
    lv.check_lengths([x for _, x in rows])
    assert {f for f, _ in rows} == set(streams.VOLUME_FAMILIES)
    low = [x for f, x in rows[:24] if f == "a"]
    assert len(low) == 2 and all(len(x) <= 100000 for x in low)
    assert info["group_collisions"] > 0, info
    # family c holds no run: nothing in it can be a run match's start (five equal bytes)
    for f, x in rows:
        if f == "c":
            assert not any(x[i] == x[i + 1] == x[i + 2] == x[i + 3] == x[i + 4] for i in range(len(x) - 4))
            break


def _volume_sample():
    """Every fifth of the corpus's streams of at most 2 000 bytes behind the long ones: about 210 streams, 150 KB"""
    rows, _ = streams.level_volume_inputs()
    return [i for i, (_, x) in enumerate(rows) if i >= 32 and len(x) <= 2000][::5]


@pytest.mark.parametrize("level", (2, 3) + LAZY)
def test_volume_sample_equals_the_model(level):
    """The models are too slow for the corpus (10 MB a level), not for a sample of its short streams: there the oracle's
    bytes over the corpus, which are what the GPU is compared with, are the model's too."""
    _, raws, _, _, out_off = lv.packed()
    ln, out, _, _ = lv.oracle_volume(level)
    model = lm if level <= 3 else zm
    sample = _volume_sample()
    assert len(sample) >= 150
    bad = [i for i in sample if out[int(out_off[i]):int(out_off[i]) + int(ln[i])].tobytes() != model.compress(raws[i], level)]
    assert not bad, (level, len(bad), bad[:8])


@pytest.mark.parametrize("level", lv.LEVELS)
def test_volume_corpus_reaches_what_it_is_for_with_the_oracle_alone(level):
    """Everything tests/test_gpu_levels_oracle.py requires of the corpus, here, so that the GPU test cannot run on inputs
    that miss a branch; a strided sample round-trips through both decoders, every stream fits its slot."""
    _, info = streams.level_volume_inputs()
    fams, raws, _, _, out_off = lv.packed()
    ln, out, c, dt = lv.oracle_volume(level)
    print("level %d: oracle over %d streams, %d bytes, 16 threads: %.2f s; counters %r" % (level, len(raws), sum(map(len, raws)), dt, c))
    assert int(ln.min()) > 0
    missed = lv.unmet_requirements(level, c, info)
    assert not missed, (level, missed)
    if level >= 4:
        assert c["max_block_symbols"] > 16384, c
    comps = []
    for i, x in enumerate(raws):
        got = out[int(out_off[i]):int(out_off[i]) + int(ln[i])].tobytes()
        assert got[:2] == b"\x78\x01" and zlib.decompress(got) == x, (level, i, fams[i], len(x))
        assert len(got) <= lv.compress_bound(len(x)) and np.all(out[int(out_off[i]) + int(ln[i]):int(out_off[i + 1])] == 0x5A), (level, i)
        comps.append(got)
    # the oracle's own decoder, as one batch over the streams packed back to back
    _, _, buf, in_off, _ = lv.packed()
    cbuf, c_off = streams.pack_exact(comps)
    back = np.zeros_like(buf)
    dl, status, _ = ob.inflate_batch(cbuf, c_off, back, in_off, nthreads=16)
    assert not status.any() and np.array_equal(dl.astype(np.uint64), np.diff(in_off)) and np.array_equal(back, buf), level
