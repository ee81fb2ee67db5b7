"""Every compression level the reference names, 0 .. 9 (the C ABI of include/fdeflate_hip_levels.h), reached as
fdeflate_amd.levels.X.

fdeflate_amd.compress_to_vec_with_level and fdeflate_amd.deflate_general_batch provide levels 0-3 and refuse the rest;
they stay as they are.  The calls here take a level: 0-3 go to those encoders and give their bytes, 4-9 run the lazy
parser with the hybrid match finder on the device (src/compress/parse/lazy.rs, src/compress/matchfinder/hybrid.rs),
bit-exact with the reference; 7, 8 and 9 are one parameter set.  No fallback where the library or the GPU is missing.
"""
import ctypes as C

from . import _lib, api

__all__ = ["LEVELS_PROVIDED", "compress_to_vec_with_level", "deflate_level_batch", "level_plan"]

LEVELS_PROVIDED = tuple(range(10))


def _level(level):
    if isinstance(level, bool) or not isinstance(level, int) or level not in LEVELS_PROVIDED:
        raise ValueError("compression level %r does not exist (levels 0 .. 9 do)" % (level,))
    return level


def compress_to_vec_with_level(data, level):
    """fdeflate::compress_to_vec_with_level (src/compress/mod.rs:299) at every level: 0 stored, 1-3 the greedy parser,
    4-9 the lazy parser (fdh_compress_to_vec_level).  Any other level: ValueError (the reference takes a u8 above 9 as
    level 7; its documentation promises 1-9)."""
    return api._compress("fdh_compress_to_vec_level", data, _level(level))


def deflate_level_batch(raw, in_off, out, out_off, level, out_len=None):
    """Encode of n buffers at `level` (fdh_deflate_level_batch): api.deflate_general_batch's contract -- device tensors,
    slots of at least api.compress_bound(len_i) bytes (level 0: api.stored_size), out_len[i] = 0xFFFFFFFF (-1) for a slot
    that is too small.  Returns when the work has finished."""
    n = in_off.numel() - 1
    out_len = api._i32(out_len, raw, n)
    api._call("fdh_deflate_level_batch", raw, in_off, out, out_off, out_len, n, _level(level))
    return out_len


def level_plan(n, cus, level):
    """(lanes, wavefronts) of the parser's launch for n streams at a lazy level, 4 .. 9, on a device of `cus` CUs
    (fdh_debug_level_plan: host arithmetic, no device)."""
    out = (C.c_uint32 * 2)()
    if _lib.lib().fdh_debug_level_plan(int(n), int(cus), _level(level), out) != 0:
        raise ValueError("no launch plan for n = %r at level %r (n >= 1, levels 4 .. 9)" % (n, level))
    return int(out[0]), int(out[1])
