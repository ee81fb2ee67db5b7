"""Helpers that the -m gpu PNG tests share: host arrays to the device, buffer layouts, row widths, environment switches
and the shapes that more than one file runs.  A plain module (no tests, no fixtures).  It needs neither the oracle nor,
until dev() is called, torch: the layout helpers are numpy alone (tests/test_png_gpu_harness.py checks them on the CPU).
"""
import numpy as np

import png_file_model as fm

GUARD = 0x5A
BAND = 64               # rows of a band: what a wavefront of the expand and pack kernels takes at a time
PASSED_ON = 77          # an upstream status: such slots are the guards between the images
# either side of a byte of 1-bit pixels, a lane's four pixels, a 16-byte store, a wavefront's 256 pixels; the bench row
EXPAND_WIDTHS = tuple(range(1, 10)) + (31, 32, 33, 63, 64, 65, 255, 256, 257, 1023)
# either side of a byte of 1-bit pixels, a lane's four pixels, a 16-byte load, a wavefront's 256 pixels; the bench row
PACK_WIDTHS = tuple(range(1, 10)) + (31, 32, 33, 63, 64, 65, 255, 256, 257, 1023)
HEIGHTS = (1, 2, 3, BAND + 1)
CHUNKS = (1, 2, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256)    # N = ceil(row_bytes / 16), as tests/test_gpu_png.py
UNIT = {1: 255, 2: 85, 4: 17, 8: 1, 16: 1}                    # a grey level of `depth` bits as an 8-bit sample


# ---- to the device ----

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(values):
    """32-bit words (statuses, palette and colour words, lengths) as the int32 tensor the calls take."""
    return dev(np.asarray(values, dtype=np.uint32).view(np.int32))


def set_env(monkeypatch, **values):
    """Sets every named variable to str(value); None deletes it."""
    for name, value in values.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


# ---- layouts ----

def offsets(sizes, front=0, slack=0):
    """Slot i holds sizes[i] + slack bytes (slack: one number, or one per slot); the first one starts `front` bytes into
    the buffer."""
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[0] = front
    off[1:] = front + np.cumsum(np.asarray(sizes, dtype=np.int64) + np.asarray(slack, dtype=np.int64))
    return off


def batch_of(files, front=5, slack=3, fill=0xEE):
    """Files one behind the other from byte `front`, `slack` fill bytes inside every slot behind the file and 16 behind
    the last slot -> (host buffer, file_off, file_len as int32)."""
    f_off = np.concatenate([[front], front + np.cumsum([len(f) + slack for f in files])]).astype(np.int64)
    host = np.full(int(f_off[-1]) + 16, fill, dtype=np.uint8)
    for o, f in zip(f_off[:-1], files):
        host[int(o):int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return host, f_off, np.array([len(f) for f in files], dtype=np.uint32).view(np.int32)


def file_slots(fd, heights, width, depth, colour, extra=0):
    """Offsets of file slots that png_file_bound says suffice, plus `extra` + 5 bytes each, from byte 3."""
    rb = fm.geometry(width, depth, colour)[0]
    sizes = [fd.png_file_bound(max(h, 1), rb) + extra + 5 for h in heights]
    return np.concatenate([[3], 3 + np.cumsum(sizes)]).astype(np.int64)


def info_rows(fd, info):
    """The scan records of a call as tuples in the order of png_file_model.Info.FIELDS."""
    f = fd.png_info_fields(info)
    return [tuple(int(f[k][i]) for k in fm.Info.FIELDS) for i in range(len(f["status"]))]


# ---- row widths ----

def widths_of(bpp, n):
    """The smallest and the largest multiple of bpp in (16 (n - 1), 16 n]: a partial and a full(est) last chunk."""
    lo, hi = 16 * (n - 1), 16 * n
    small, large = (lo // bpp + 1) * bpp, hi // bpp * bpp
    assert lo < small < large <= hi and (small + 15) // 16 == n == (large + 15) // 16
    return small, large


def widths_above(bpp, gate):
    """The first multiple of bpp above `gate` (the last row width of a kernel's one-step path), and two far above."""
    first = (gate // bpp + 1) * bpp
    assert first > gate and first - bpp <= gate
    return first, 5760, 15360


# ---- pictures ----

def random_rgba(r, width, height, depth, colour):
    """Random pixel words (uint32 [height * width]) that the pair holds without loss (not colour type 3)."""
    n = width * height
    if colour in (0, 4):
        g = r.integers(0, 1 << min(depth, 8), n).astype(np.uint32) * UNIT[depth]
        rgb = g * 0x010101
    else:
        rgb = r.integers(0, 1 << 24, n).astype(np.uint32)
    alpha = r.integers(0, 256, n).astype(np.uint32) if colour in (4, 6) else np.full(n, 255, dtype=np.uint32)
    return rgb | alpha << 24
