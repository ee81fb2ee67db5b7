"""Payloads that drive Adler-32 to its largest sums, the streams that carry them, and the reference sum.

Every kernel of the library defers the modulo of its Adler-32 accumulators and is right only while they stay below a
bound (DESIGN.md "Adler-32 accumulators").  Bytes of 0xFF reach those bounds first; uniform random bytes reach half of
them.  Used by tests/test_adler_payloads.py (CPU) and tests/test_gpu_adler.py."""
import functools
import zlib

import numpy as np

import oracle_binding as ob

MOD = 65521

LENGTHS = (1, 15, 16, 17, 2047, 2048, 2049, 4097, 65535, 65536, 65537, 131071, 131072, 131073, 46764, 250000,
           (1 << 20) + 3, (1 << 22) + 5)
# after 46 764 bytes of 0xFF both halves are 65 520, the largest state there is; again every 65 521 bytes
MAXIMAL_STATE_LENGTHS = (46764, 46764 + MOD)


def adler32_model(data, state=1):
    """Adler-32 in plain integers, a byte at a time, reduced at every step (RFC 1950, 8.2)."""
    a, b = state & 0xFFFF, state >> 16
    for x in bytes(data):
        a = (a + x) % MOD
        b = (b + a) % MOD
    return b << 16 | a


def _high(n, seed):
    return np.random.default_rng(seed).integers(0xF8, 0x100, n, dtype=np.uint8)


def ff(n):
    """n bytes of 0xFF: the worst case of A, of B and of the offset sums."""
    return b"\xff" * n


def high(n):
    """Uniform in 0xF8 .. 0xFF (mean 251.5, 98.6 % of the worst case), no long runs of equal literals."""
    return _high(n, 0xAD1E).tobytes()


def ff_sparse(n):
    """`high` with about half of the bytes zeroed, in stretches of 1 .. 600 bytes between kept stretches of 1 .. 600."""
    r = np.random.default_rng(0x5BA5)
    x = _high(n, 0xAD1F)
    lens = r.integers(1, 601, 2 * (n // 300 + 2))
    keep = np.repeat(np.arange(lens.size) & 1, lens)[:n].astype(bool)    # starts with a zero stretch
    assert keep.size == n
    x[~keep] = 0
    return x.tobytes()


def ff_front(n):
    """`high` in the first quarter, zeros behind: the largest weights `total - offset` lie on the heavy bytes."""
    q = (n + 3) // 4
    return _high(q, 0xAD20).tobytes() + bytes(n - q)


def ff_back(n):
    """`high` in the last quarter, zeros in front: the largest weights lie on the zeros."""
    q = (n + 3) // 4
    return bytes(n - q) + _high(q, 0xAD21).tobytes()


PAYLOADS = {"ff": ff, "high": high, "ff_sparse": ff_sparse, "ff_front": ff_front, "ff_back": ff_back}


def _zlib_strategy(strategy):
    def enc(raw):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, strategy)
        return c.compress(raw) + c.flush()
    return enc


ENCODINGS = {
    "uf": ob.compress_ultra_fast, "stored": ob.compress_stored, "level1": ob.compress_level1, "rle": ob.compress_rle,
    "zlib0": lambda raw: zlib.compress(raw, 0), "zlib1": lambda raw: zlib.compress(raw, 1),
    "zlib6": lambda raw: zlib.compress(raw, 6), "zlib9": lambda raw: zlib.compress(raw, 9),
    "huff": _zlib_strategy(zlib.Z_HUFFMAN_ONLY), "fixed": _zlib_strategy(zlib.Z_FIXED),
}
ULTRAFAST_FORMAT = ("uf",)                                   # what the landing decoder and the interval kernel take
LZ_FORMAT = ("level1", "zlib1", "zlib6", "zlib9")            # what the LZ-window kernel must take


@functools.lru_cache(maxsize=None)
def payload(kind, n):
    return PAYLOADS[kind](n)


@functools.lru_cache(maxsize=None)
def stream(kind, n, encoding):
    return ENCODINGS[encoding](payload(kind, n))


def cases(lengths=LENGTHS, kinds=tuple(PAYLOADS), encodings=tuple(ENCODINGS)):
    """-> list of (name, stream, raw), name = "<payload>_<length>_<encoding>" """
    return [("%s_%d_%s" % (k, n, e), stream(k, n, e), payload(k, n)) for k in kinds for n in lengths for e in encodings]
