"""The volume corpus of encoder levels 2..9 (streams.level_volume_inputs) through the oracle, once per process and level,
and what the corpus is required to reach, for tests/test_oracle_levels.py (CPU) and tests/test_gpu_levels_oracle.py (GPU):
both ask the same list, so the GPU test never runs on inputs that the CPU test has not shown to reach every branch."""
import time

import numpy as np

import oracle_binding as ob
import streams

LEVELS = (2, 3, 4, 5, 6, 7, 8, 9)
DEPTH = {2: 16, 3: 16, 4: 16, 5: 64, 6: 128, 7: 256, 8: 256, 9: 256}    # search_depth, compress/mod.rs:78-87
FINDER_EXITS = ("steps2", "nice", "eod", "depth", "alias")
HYBRID_EXITS = ("quarter", "rescue_hit", "rescue_miss", "rescue_zero")
LOOP_CLAUSES = ("m0_empty", "m0_earlier", "m0_longer", "m0_kept", "m0_inserted", "m0_cut", "m0_dropped", "m2_same_start")
INPUT_COUNTERS = ("skip_nonzero", "scan_end_in_skip", "rle_events")
GUARD = 5       # bytes behind every stream's bound, as test_lazy_levels_bit_exact has them

_packed = None
_results = {}


def compress_bound(n):
    """fdh_compress_bound (include/fdeflate_hip.h), as arithmetic: no library, no GPU."""
    return n + n // 2 + 1024


def packed():
    """-> (families, raws, in_buf, in_off, out_off): the corpus back to back, and slots of compress_bound + GUARD bytes"""
    global _packed
    if _packed is None:
        rows, _ = streams.level_volume_inputs()
        raws = [x for _, x in rows]
        buf, in_off = streams.pack_exact(raws)
        out_off = np.zeros(len(raws) + 1, dtype=np.int64)
        out_off[1:] = np.cumsum([compress_bound(len(x)) + GUARD for x in raws])
        _packed = ([f for f, _ in rows], raws, buf, in_off, out_off)
    return _packed


def oracle_volume(level):
    """-> (out_len, out_buf, counters, seconds): ob.deflate_level_batch over the corpus on 16 threads, the output buffer
    filled with 0x5A first so that it can be compared whole with the device's"""
    if level not in _results:
        _, _, buf, in_off, out_off = packed()
        out = np.full(int(out_off[-1]), 0x5A, dtype=np.uint8)
        ob.level_counters_reset()
        t0 = time.perf_counter()
        ln = ob.deflate_level_batch(buf, in_off, out, out_off.astype(np.uint64), level, 16)
        dt = time.perf_counter() - t0
        _results[level] = (ln, out, ob.level_counters(reset=True), dt)
    return _results[level]


def unmet_requirements(level, c, info):
    """What the corpus is for, as a list of the conditions it misses at `level` (empty: all met).  c: the oracle's
    counters over the whole batch; info: level_volume_inputs()'s."""
    missed = []

    def need(ok, what):
        if not ok:
            missed.append(what)

    names = FINDER_EXITS + (HYBRID_EXITS + LOOP_CLAUSES if level >= 4 else ()) + INPUT_COUNTERS
    for k in names:
        need(c[k] > 0, "%s == 0" % k)
    need(c["maxsteps"] == DEPTH[level], "maxsteps %d != search_depth %d" % (c["maxsteps"], DEPTH[level]))
    need(c["blocks"] > 0, "no block cut before the end")
    need(c["pass2_base"] > 32768, "pass2_base %d: no second pass that starts past the window" % c["pass2_base"])
    need(c["pending"] == c["resumed"] > 0, "pending %d, resumed %d" % (c["pending"], c["resumed"]))
    need(info["group_collisions"] > 0, "no two steps of one look-ahead group share a table index")
    return missed


def mismatches_against_oracle(raw, comp, clen, bound, level):
    """For the scale tests: `raw` an [n, L] uint8 tensor on the device, `comp` the device's n slots of `bound` bytes,
    `clen` its lengths.  Every stream goes through the oracle on 16 threads into the same slot layout; the comparison
    of the bytes in front of each stream's end is done on the device.  -> (indices of the streams that differ in length
    or bytes, the oracle's seconds)"""
    import torch
    n, L = raw.shape
    h_raw = raw.cpu().numpy().reshape(-1)
    in_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    out_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(bound)
    want = np.zeros(n * bound, dtype=np.uint8)
    t0 = time.perf_counter()
    want_len = ob.deflate_level_batch(h_raw, in_off, want, out_off, level, 16)
    dt = time.perf_counter() - t0
    assert int(want_len.min()) > 0
    d_want_len = torch.from_numpy(want_len.astype(np.int64)).cuda()
    got_len = clen.to(torch.int64) & 0xFFFFFFFF
    bad = got_len != d_want_len
    rows = 1024     # slots per comparison, so that the temporaries stay small
    for r0 in range(0, n, rows):
        r1 = min(r0 + rows, n)
        w = torch.from_numpy(want[r0 * bound:r1 * bound]).cuda().view(r1 - r0, bound)
        g = comp[r0 * bound:r1 * bound].view(r1 - r0, bound)
        inside = torch.arange(bound, device="cuda")[None, :] < d_want_len[r0:r1, None]
        bad[r0:r1] |= ((g != w) & inside).any(dim=1)
        if r0 == 0:     # the comparison's own control: the oracle's first stream with its last byte changed must differ
            probe = w[:1].clone()
            probe[0, int(want_len[0]) - 1] ^= 0xFF
            assert bool(((probe != w[:1]) & inside[:1]).any()) and not bool(((w[:1] != w[:1]) & inside[:1]).any())
    return torch.nonzero(bad).flatten().cpu().tolist(), dt


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))[0]
    return int(d[0]) if d.size else n


def gpu_compare_with_oracle(level, pick, what):
    """The streams `pick` (indices into the corpus, None: all) as one batch through levels.deflate_level_batch, guard
    bytes 0x5A behind every stream; lengths, bytes and guards against the oracle's."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import levels
    fams, raws, buf, in_off, out_off = packed()
    want_len, want_out, _, _ = oracle_volume(level)
    if pick is None:
        pick = np.arange(len(raws))
        b, i_off, o_off = buf, in_off.astype(np.int64), out_off
    else:
        b, i_off = streams.pack_exact([raws[i] for i in pick])
        i_off = i_off.astype(np.int64)
        o_off = np.zeros(len(pick) + 1, dtype=np.int64)
        o_off[1:] = np.cumsum([compress_bound(len(raws[i])) + GUARD for i in pick])
    assert all(fd.compress_bound(len(raws[i])) == compress_bound(len(raws[i])) for i in pick[:40])
    d_in, d_in_off, d_out_off = torch.from_numpy(b).cuda(), torch.from_numpy(i_off).cuda(), torch.from_numpy(o_off).cuda()
    d_out = torch.full((int(o_off[-1]),), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ln = levels.deflate_level_batch(d_in, d_in_off, d_out, d_out_off, level)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ln = ln.cpu().numpy().view(np.uint32)
    h = d_out.cpu().numpy()
    print("level %d, %s: %d streams, %d bytes on the device in %.2f s" % (level, what, len(pick), int(i_off[-1]), dt))
    for k, i in enumerate(pick):
        w0 = int(out_off[i])
        want = want_out[w0:w0 + int(want_len[i])]
        slot = h[int(o_off[k]):int(o_off[k + 1])]
        got = slot[:min(int(ln[k]), slot.size)]
        if int(ln[k]) != int(want_len[i]) or not np.array_equal(got, want):
            raise AssertionError("level %d (%s): stream %d, family %s, %d bytes: %d compressed bytes, the oracle has %d; first "
                                 "difference at byte %d" % (level, what, i, fams[i], len(raws[i]), int(ln[k]), int(want_len[i]),
                                                           _first_difference(got.tobytes(), want.tobytes())))
        assert np.all(slot[int(ln[k]):] == 0x5A), "level %d (%s): stream %d, family %s, %d bytes: wrote behind its stream" % (
            level, what, i, fams[i], len(raws[i]))


def check_lengths(raws):
    """The lengths the corpus promises: every length 0..300, two dozen long streams, none above 160 000."""
    lens = sorted(len(x) for x in raws)
    missed = [n for n in range(301) if n not in set(lens)]
    long_ones = [n for n in lens if n >= 40000]
    assert not missed, missed
    assert 20 <= len(long_ones) <= 28 and lens[-1] <= 160000, long_ones
    assert all(n <= 20000 for n in lens if n < 40000)
