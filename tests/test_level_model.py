"""CPU checks of tests/level_model.py, the pure-Python restatement that supplies the expected bytes of
encoder levels 2 and 3, and of the level-selecting entry point's behaviour without a GPU.

- the pin: the model equals the oracle, byte for byte, at level 1 and in RLE mode over the oracle
  tests' encoder inputs and the run-edge inputs -- parser, runs, match_length::<true>, block cutting,
  the block writer;
- levels 2 and 3 round-trip through zlib and stay inside fdh_compress_bound's formula;
- the chain inputs reach every exit of the chain search at both levels (coverage is asserted, not hoped
  for).  The chain finder and match_length::<false> against the oracle's own statement of them: tests/test_oracle_levels.py;
- the inputs reach every exit of the device's counter of equal bytes in each of its four uses;
- the general encoder's launch plan (lanes, wavefronts), through the library's hook: no device needed.
"""
import ctypes as C
import zlib

import pytest

import level_model as lm
import oracle_binding as ob
import streams


def compress_bound(n):
    """fdh_compress_bound (include/fdeflate_hip.h), as arithmetic: no library, no GPU."""
    return n + n // 2 + 1024


def test_model_is_pinned_by_the_oracle_at_level1_and_rle():
    res = lm.oracle_level_results()
    assert len(res["inputs"]) == len(streams.encoder_inputs()) + 3948 + 24
    for i, x in enumerate(res["inputs"]):
        assert res[1][i] == ob.compress_level1(x), ("level 1", i, len(x))
        assert res["rle"][i] == ob.compress_rle(x), ("rle", i, len(x))


def test_model_empty_input_kat():
    for level in (1, 2, 3):
        assert lm.compress(b"", level) == bytes.fromhex("7801030000000001")
    assert lm.compress_rle(b"") == bytes.fromhex("7801030000000001")


@pytest.mark.parametrize("level", [2, 3])
def test_levels_2_and_3_round_trip_and_fit_the_bound(level):
    for i, (x, out, _) in enumerate(lm.model_results()[level]):
        assert out[:2] == b"\x78\x01", (level, i)
        assert zlib.decompress(out) == x, (level, i, len(x))
        assert len(out) <= compress_bound(len(x)), (level, i, len(x), len(out))


@pytest.mark.parametrize("level", [2, 3])
def test_chain_inputs_reach_every_exit_of_the_search(level):
    tot = dict(steps2=0, nice=0, eod=0, depth=0, alias=0, unwritten=0, maxsteps=0)
    for _, _, c in lm.model_results()[level]:
        for k, v in c.items():
            tot[k] = max(tot[k], v) if k == "maxsteps" else tot[k] + v
    print("level %d chain counters: %r" % (level, tot))
    for k in ("steps2", "nice", "eod", "depth", "alias"):
        assert tot[k] > 0, (level, k, tot)
    assert tot["maxsteps"] == 16, (level, tot)
    assert tot["unwritten"] == 0, (level, tot)


def test_inputs_reach_every_exit_of_the_counter_of_equal_bytes():
    """encoder_inputs() + chain_inputs() + run_edge_inputs() at levels 2 and 3, the first and the last of them at
    level 1 and RLE as well: each of the counter's four uses ends at a difference in a group of 32, in a group of 8,
    in the wide tail and in the byte tail, and at its limit."""
    tot = lm.model_results()["exits"] + lm.oracle_level_results()["exits"]
    for use in lm.USES:
        print("%-10s %s" % (use, "  ".join("%s %d" % (e, tot[use, e]) for e in lm.EXITS)))
    for use in lm.USES:
        for e in lm.EXITS:
            assert tot[use, e] > 0, (use, e)


def _general_plan(n, mode, cus=256):
    from fdeflate_amd import _lib
    out = (C.c_uint32 * 2)()
    assert _lib.lib().fdh_debug_general_plan(C.c_uint64(n), C.c_int(cus), C.c_uint32(mode), out) == 0
    return out[0], out[1]


def test_general_plan_is_pinned(monkeypatch):
    """(lanes, wavefronts) of the parser's launch on 256 CUs.  By hand: lanes halve from 64 down to 4 while
    ceil(n / lanes) is below 256 x 8 = 2 048 wavefronts at level 1, 256 x 16 = 4 096 otherwise; the wavefronts are
    ceil(n / lanes), at most (streams resident) / lanes, where 16 GiB of tables hold 65 536 streams at level 1
    (256 KiB each), 43 690 at levels 2 and 3 (384 KiB), and RLE has no tables."""
    import fdeflate_amd as fd
    monkeypatch.delenv("FDH_GEN_LANES", raising=False)
    monkeypatch.delenv("FDH_GEN_RESIDENT", raising=False)
    assert _general_plan(1, fd.MODE_LEVEL1) == (4, 1)
    assert _general_plan(8192, fd.MODE_LEVEL1) == (4, 2048)
    assert _general_plan(65536, fd.MODE_LEVEL1) == (32, 2048)
    assert _general_plan(200000, fd.MODE_LEVEL1) == (64, 1024)      # 3 125 wanted, 65 536 / 64 resident
    assert _general_plan(65536, fd.MODE_RLE) == (16, 4096)
    assert _general_plan(1000000, fd.MODE_RLE) == (64, 15625)
    assert _general_plan(65536, fd.MODE_LEVEL2) == (16, 2730)       # 43 690 / 16
    assert _general_plan(100, fd.MODE_LEVEL3) == (4, 25)
    monkeypatch.setenv("FDH_GEN_LANES", "1")
    assert _general_plan(70, fd.MODE_LEVEL1) == (1, 70)
    monkeypatch.setenv("FDH_GEN_LANES", "16")
    monkeypatch.setenv("FDH_GEN_RESIDENT", "64")
    assert _general_plan(100, fd.MODE_LEVEL2) == (16, 4)            # ceil(100 / 16) = 7 wanted, 64 / 16 resident
    from fdeflate_amd import _lib
    assert "fdh_debug_general_plan" not in _lib.SIGNATURES


def test_level_entry_point_refuses_levels_not_provided():
    """Level 4 and above: ValueError before the library is touched, GPU or not."""
    import fdeflate_amd as fd
    for level in (4, 9, -1, 256, True, 2.0, None):
        with pytest.raises(ValueError):
            fd.compress_to_vec_with_level(b"x", level)
    assert (fd.MODE_LEVEL1, fd.MODE_RLE, fd.MODE_LEVEL2, fd.MODE_LEVEL3) == (1, 2, 3, 4)


def test_level_entry_point_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import fdeflate_amd as fd
    from fdeflate_amd._lib import FdeflateHipError
    for level in (0, 1, 2, 3):
        with pytest.raises(FdeflateHipError):
            fd.compress_to_vec_with_level(b"x", level)
