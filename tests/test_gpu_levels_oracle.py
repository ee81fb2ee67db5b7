"""-m gpu: encoder levels 2..9 on the GPU against the oracle's C restatement of the same levels (oracle/fdeflate_oracle.c),
bit-exact over the volume corpus: streams.level_volume_inputs(), 2 000 streams and 10.3 MB per level from eight families
made for what the kernels can get wrong (equal hashes inside one look-ahead group, the skip-ahead leaving the scan range
inside a group, runs next to table candidates, the window edge, link rings that a longer stream left behind).
tests/test_oracle_levels.py pins the oracle against both Python models, bytes and branch counts, and shows on the CPU
that the corpus reaches every branch asked for here (level_volume.unmet_requirements).

One batch per test.  Measured, per level 2 / 3 / 4 / 5 / 6 / 7 / 8 / 9: the oracle's side, 16 threads on the 8 cores of
the build machine, 0.14 / 0.15 / 0.25 / 0.30 / 0.28 / 0.07 / 0.07 / 0.07 s (the longest stream, not the sum, decides);
the device's side on an MI355X, launch to synchronize: the library's own shape 0.10 / 0.16 / 0.22 / 0.35 / 0.70 /
1.03 / 1.07 / 1.02 s, 16 lanes with 64 resident 0.39 / 0.50 / 0.95 / 1.35 / 2.30 / 2.93 / 3.21 / 2.92 s, the 256-stream
subset at most 2.5 s (1 lane) and 1.95 s (64 lanes).  The 40 tests of the module took 36 s together, the slowest 3.2 s.
With 2 000 streams both sides stay within a few seconds, so the count was left at the starting point.
"""
import numpy as np
import pytest

import level_volume as lv
import streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gpu_harness
    return gpu_harness


_run_and_compare = lv.gpu_compare_with_oracle


def _env(monkeypatch, lanes=None, resident=None):
    for name, v in (("FDH_GEN_LANES", lanes), ("FDH_GEN_RESIDENT", resident)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


@pytest.mark.parametrize("level", lv.LEVELS)
def test_volume_bit_exact(harness, level, monkeypatch):
    """The whole corpus in the library's own launch shape."""
    _env(monkeypatch)
    _run_and_compare(level, None, "own launch shape")


@pytest.mark.parametrize("level", lv.LEVELS)
def test_volume_tables_reused(harness, level, monkeypatch):
    """16 lanes, 64 streams resident: every wavefront takes 31 further rounds.  The corpus begins with its long streams,
    so the first round leaves 160 000-byte streams' links under every slot of the rings, which are not cleared, and
    every later stream is shorter than the one whose tables it inherits."""
    _env(monkeypatch, lanes=16, resident=64)
    _run_and_compare(level, None, "16 lanes, 64 resident")


def _subset():
    """256 streams: the long ones, the clause inputs and 224 of the rest, every seventh (each family in turn)"""
    n = len(lv.packed()[1])
    rest = list(range(32, n, 7))
    return np.asarray(list(range(32)) + rest[:224])


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("level", lv.LEVELS)
def test_volume_lane_shapes(harness, level, lanes, monkeypatch):
    pick = _subset()
    assert pick.size == 256 and len({lv.packed()[0][i] for i in pick}) == 8
    _env(monkeypatch, lanes=lanes)
    _run_and_compare(level, pick, "%d lanes" % lanes)


@pytest.mark.parametrize("level", lv.LEVELS)
def test_volume_inputs_reach_what_they_are_for(harness, level):
    """With the oracle's counters over the batch: every exit of the finder and (levels 4..9) every clause of the lazy
    loop, a walk as long as the level's depth, a block cut in the first pass and a second pass that starts past the
    window, a pending match resumed, skip-ahead steps, a scan range that ends inside a skip, runs, and steps of one
    look-ahead group that share a table index.  Requirements, not tendencies: tests/test_oracle_levels.py has shown them
    on the CPU."""
    _, info = streams.level_volume_inputs()
    _, _, c, dt = lv.oracle_volume(level)
    print("level %d: oracle %.2f s, counters %r, %r" % (level, dt, c, info))
    missed = lv.unmet_requirements(level, c, info)
    assert not missed, (level, missed)
    lv.check_lengths(lv.packed()[1])
