#!/usr/bin/env python3
"""What the encoder's doors refuse, call by call: one line `call(arguments) -> return code, fdh_last_error()` for
fdh_deflate_general_batch, fdh_deflate_level_batch, fdh_deflate_level_pieces_batch, fdh_compress_to_vec_with_level and
fdh_compress_to_vec_level over modes / levels, batch sizes and null pointers.  For comparing two builds of the library:

    python tools/refusals.py > after.txt;  FDH_LIB=/other/libfdeflate_hip.so python tools/refusals.py > before.txt

Runs on a machine WITHOUT a GPU only: there every refusal comes before the device check, and the calls that pass every
check end as "no HIP device".  With a device those calls would be launched on the host memory that stands in for the
pointers here, so the script stops instead."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdeflate_amd import _lib  # noqa: E402

L = _lib.lib()
if L.fdh_device_count() > 0:
    sys.exit("a HIP device is present: this table is made on a machine without one")

_meta = (ctypes.c_uint64 * 8)()
P = ctypes.cast(_meta, ctypes.c_void_p)     # host memory standing in for a pointer: refused before it is looked at
COUNTS = (0, 1, 1 << 31)
# in, in_off, out, out_off, out_len
POINTERS = {"all null": (None,) * 5, "null metadata": (P, None, P, None, None), "null out": (P, P, None, P, P), "none null": (P,) * 5}


def line(call, what, rc):
    print("%s(%s) -> %d, %r" % (call, what, rc, L.fdh_last_error().decode() if rc else ""))


for mode in (0, 1, 2, 3, 4, 5, 0xFFFFFFFF):
    for n in COUNTS:
        for name, (a, a_off, o, o_off, o_len) in POINTERS.items():
            line("fdh_deflate_general_batch", "mode %d, n %d, %s" % (mode, n, name), L.fdh_deflate_general_batch(a, a_off, o, o_off, o_len, n, mode, None))
for level in (*range(11), 0xFFFFFFFF):
    for n in COUNTS:
        for name, (a, a_off, o, o_off, o_len) in POINTERS.items():
            line("fdh_deflate_level_batch", "level %d, n %d, %s" % (level, n, name), L.fdh_deflate_level_batch(a, a_off, o, o_off, o_len, n, level, None))
for level in range(11):
    for n in COUNTS:
        for name, (a, a_off, o, o_off, o_len) in POINTERS.items():
            for last, adler in ((P, P), (None, P), (P, None), (None, None)):
                what = "level %d, n %d, %s, piece_last %s, piece_adler %s" % (level, n, name, "set" if last else "null", "set" if adler else "null")
                line("fdh_deflate_level_pieces_batch", what, L.fdh_deflate_level_pieces_batch(a, a_off, last, o, o_off, o_len, adler, n, level, None))
for call in ("fdh_compress_to_vec_with_level", "fdh_compress_to_vec_level"):
    for level in range(11):
        for data in (b"", b"abc"):
            for results in ("set", "null"):
                out, size = ctypes.c_void_p(), ctypes.c_size_t()
                args = (ctypes.byref(out), ctypes.byref(size)) if results == "set" else (None, None)
                rc = getattr(L, call)(data, len(data), level, *args)
                line(call, "level %d, %d bytes, result pointers %s" % (level, len(data), results), rc)
                assert not out.value
