"""CPU checks of tests/lazy_model.py, the pure-Python restatement that supplies the expected bytes of encoder levels 4-9
(LazyParser + HybridMatchFinder) next to the oracle's C restatement of the same levels, and of the lazy levels' launch plan.

- every output round-trips through zlib and the oracle's decoder, starts 78 01 and fits fdh_compress_bound's formula;
- the empty input, levels 7 = 8 = 9;
- coverage is asserted, not hoped for: at each of the levels 4, 5, 6 and 9 the inputs reach every exit of the hybrid
  search (both outcomes of the 4-table's rescue, the depth cut to a quarter, nice_length, end of data, the depth, the
  alias at distance 32 768), every clause of the lazy loop (m0 replaced because it is empty / m1 starts earlier / m1
  starts at the same place and is longer, m0 inserted shortened and m0 dropped), a first pass that ends with a pending
  m1, a first pass that writes a block so that the second starts past 0, and a block of more than 16 384 symbols;
- no link slot is read before the stream has written it (the device does not clear the ring);
- level 6 against level 3 in size, as a sanity condition on the model;
- fdh_debug_level_plan on 256 CUs against the rule worked by hand.
lazy_model.Hybrid and lazy_model.LazyParser.compress against the second reading of the Rust, the oracle's: bytes and
branch counts, in tests/test_oracle_levels.py.  The real crate still cannot be run here.
"""
import ctypes as C
import zlib

import pytest

import lazy_model as zm
import level_model as lm
import oracle_binding as ob
import streams

LEVELS = (4, 5, 6, 9)
EMPTY = bytes.fromhex("7801030000000001")


def compress_bound(n):
    """fdh_compress_bound (include/fdeflate_hip.h), as arithmetic: no library, no GPU."""
    return n + n // 2 + 1024


@pytest.mark.parametrize("level", LEVELS)
def test_lazy_levels_round_trip_and_fit_the_bound(level):
    for i, (x, out, _) in enumerate(zm.model_results()[level]):
        assert out[:2] == b"\x78\x01", (level, i)
        assert zlib.decompress(out) == x, (level, i, len(x))
        st, back, _ = ob.decompress_bounded(out, len(x))
        assert st == 0 and back == x, (level, i, len(x), st)
        assert len(out) <= compress_bound(len(x)), (level, i, len(x), len(out))


def test_model_empty_input_kat_and_refused_levels():
    for level in range(4, 10):
        assert zm.compress(b"", level) == EMPTY
    for level in (3, 10, True, 6.0, None):
        with pytest.raises(ValueError):
            zm.compress(b"x", level)


def test_levels_7_8_and_9_are_one_parameter_set():
    assert zm.PARAMS[7] is zm.PARAMS[8] is zm.PARAMS[9]
    for x in zm.lazy_inputs()[1:] + streams.late_match_inputs()[:4]:
        assert zm.compress(x, 7) == zm.compress(x, 8) == zm.compress(x, 9)


def _totals(level):
    tot = {}
    for _, _, c in zm.model_results()[level]:
        zm.add_counters(tot, c)
    return tot


@pytest.mark.parametrize("level", LEVELS)
def test_inputs_reach_every_exit_of_the_search_and_every_branch_of_the_loop(level):
    tot = _totals(level)
    print("level %d counters: %r" % (level, tot))
    assert set(tot) == set(zm.FINDER_COUNTERS + zm.LOOP_COUNTERS)
    for k in ("steps2", "nice", "eod", "depth", "alias", "quarter", "rescue_hit", "rescue_miss", "rescue_zero"):
        assert tot[k] > 0, (level, k, tot)
    assert tot["maxsteps"] == zm.PARAMS[level][2][1], (level, tot)     # a walk as long as search_depth
    assert tot["unwritten"] == 0, (level, tot)
    for k in ("m0_empty", "m0_earlier", "m0_longer", "m0_kept", "m0_inserted", "m0_cut", "m0_dropped", "m2_same_start"):
        assert tot[k] > 0, (level, k, tot)
    assert tot["pending"] > 0 and tot["resumed"] == tot["pending"], (level, tot)   # every pending m1 is resumed, not searched again
    assert tot["blocks"] > 0 and tot["max_block_symbols"] > lm.BLOCK_SYMBOLS, (level, tot)
    assert tot["pass2_base"] > 0, (level, tot)


@pytest.mark.parametrize("level", LEVELS)
def test_short_chain_input_cuts_a_block_in_the_first_pass_without_long_walks(level):
    """lazy_model.short_chain_input(): the first pass writes a block (so the second starts past 0 with base_index > 0),
    there is a deferral past position 32 768, and the walks are short: fewer than one further candidate per four
    bytes (a candidate at exactly ip - 32768 still goes round until the depth is used up)."""
    rows = zm.model_results()[level]
    x = zm.short_chain_input()
    assert 50000 <= len(x) <= 120000
    c = next(c for y, _, c in rows if y == x)
    assert c["blocks"] >= 1 and c["pass2_base"] > 32768 and c["m0_empty"] > 100 and c["steps2"] < len(x) // 4, (level, c)


def test_level_6_is_not_larger_than_level_3_where_short_far_matches_pay():
    """A sanity condition on the model, over streams.encoder_inputs().  It does NOT hold for the whole set: on three
    inputs level 6 is larger than level 3 -- 50 000 bytes of noise over five symbols (+2 %) and the two synthetic
    PNG-filter streams of seeds 0 and 7 (+14 %, +13 %).  Level 6 has min_match 4: where the walk finds nothing its
    4-table admits a 4-byte match at any distance up to 32 768, which on such data costs more bits than the four
    literals it replaces; level 3 takes nothing below 6 bytes.  On every other input level 6 is not larger, and in
    total over those it is smaller."""
    enc = streams.encoder_inputs()
    sizes6 = {x: len(o) for x, o, _ in zm.model_results()[6]}
    sizes3 = {x: len(o) for x, o, _ in lm.model_results()[3]}
    worse = [i for i, x in enumerate(enc) if len(x) != 300000 and sizes6[x] > sizes3[x]]     # (the 300 000-byte input is not in level 6's set)
    for i, x in enumerate(enc):
        if len(x) != 300000:
            print("input %2d: %6d bytes, level 3 %6d, level 6 %6d" % (i, len(x), sizes3[x], sizes6[x]))
    assert worse == [8, 17, 18], worse
    rest = [x for i, x in enumerate(enc) if i not in worse and len(x) != 300000]
    assert sum(sizes6[x] for x in rest) < sum(sizes3[x] for x in rest)


def _plan(n, level, cus=256):
    from fdeflate_amd import _lib
    out = (C.c_uint32 * 2)()
    rc = _lib.lib().fdh_debug_level_plan(C.c_uint64(n), C.c_int(cus), C.c_uint32(level), out)
    return (out[0], out[1]) if rc == 0 else rc


def test_level_plan_is_pinned(monkeypatch):
    """(lanes, wavefronts) of the lazy parser's launch on 256 CUs.  By hand: lanes halve from 64 down to 4 while
    ceil(n / lanes) is below 256 x 16 = 4 096 wavefronts; the wavefronts are ceil(n / lanes), at most (streams resident)
    / lanes, where 16 GiB of tables hold 26 214 streams of 640 KiB each."""
    from fdeflate_amd import levels
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    assert _plan(1, 4) == (4, 1)
    assert _plan(100, 6) == (4, 25)
    assert _plan(8192, 6) == (4, 2048)
    assert _plan(65536, 6) == (16, 1638)            # 4 096 wanted, 26 214 / 16 resident
    assert _plan(1000000, 9) == (64, 409)           # 26 214 / 64
    for level in (4, 5, 7, 8):
        assert _plan(65536, level) == (16, 1638)
    for level in (0, 3, 10):
        assert _plan(100, level) == -1
    assert _plan(0, 6) == -1
    assert levels.level_plan(65536, 256, 6) == (16, 1638)
    monkeypatch.setenv("FDH_GEN_LANES", "1")
    assert _plan(70, 5) == (1, 70)
    monkeypatch.setenv("FDH_GEN_LANES", "16")
    monkeypatch.setenv("FDH_GEN_RESIDENT", "64")
    assert _plan(100, 6) == (16, 4)                 # ceil(100 / 16) = 7 wanted, 64 / 16 resident
