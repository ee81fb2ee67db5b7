"""CPU checks of tests/level_model.py, the pure-Python restatement that supplies the expected bytes of
encoder levels 2 and 3 (the oracle has level 1 and RLE only), and of the level-selecting entry point's
behaviour without a GPU.

- the pin: the model equals the oracle, byte for byte, at level 1 and in RLE mode over the oracle
  tests' encoder inputs -- parser, runs, match_length::<true>, block cutting, the block writer;
- levels 2 and 3 round-trip through zlib and stay inside fdh_compress_bound's formula;
- the chain inputs reach every exit of the chain search at both levels (coverage is asserted, not hoped
  for).  What stays unpinned by a second implementation is the chain finder and match_length::<false>.
"""
import zlib

import pytest

import level_model as lm
import oracle_binding as ob
import streams


def compress_bound(n):
    """fdh_compress_bound (include/fdeflate_hip.h), as arithmetic: no library, no GPU."""
    return n + n // 2 + 1024


def test_model_is_pinned_by_the_oracle_at_level1_and_rle():
    for i, x in enumerate(streams.encoder_inputs()):
        assert lm.compress(x, 1) == ob.compress_level1(x), ("level 1", i, len(x))
        assert lm.compress_rle(x) == ob.compress_rle(x), ("rle", i, len(x))


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
