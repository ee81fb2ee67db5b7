"""The expected bytes of include/fdeflate_hip_pieces.h, from the encoder models as they are: level_model.compress for
levels 1-3 and lazy_model.compress for levels 4-9 give a slice's zlib stream, and level_model.write_block -- wrapped for
the duration of one call, never edited -- tells where every block starts and whether it carries BFINAL.  A piece is the
stream without 78 01 and the Adler-32: as it stands for a last piece; for a non-last piece with every BFINAL cleared
and, behind the last block's last bit, write_bits(0, 3), the padding and 00 00 FF FF (Flush::Sync, reference
src/compress/mod.rs:284-287).  The stitched stream is 78 01, the pieces, the Adler-32 of the whole input.
"""
import functools
import zlib

import numpy as np

import lazy_model
import level_model

MOD = 65521
SYNC = b"\x00\x00\xff\xff"


def encode_slice(data, level):
    """(zlib stream of `data` at `level`, [(first bit, bit behind the last, eof)] of its blocks), the positions counted
    from the stream's first byte.  The empty input has no block: its 03 00 is written without write_block."""
    blocks = []
    real = level_model.write_block

    def recording(w, whole, symbols, eof):
        start = 8 * len(w.out) + w.nbits
        real(w, whole, symbols, eof)
        blocks.append((start, 8 * len(w.out) + w.nbits, bool(eof)))

    level_model.write_block = recording
    try:
        stream = level_model.compress(data, level) if level <= 3 else lazy_model.compress(data, level)
    finally:
        level_model.write_block = real
    return stream, blocks


def piece(data, level, last):
    """The raw-deflate piece of the slice `data`."""
    return piece_of(*encode_slice(bytes(data), level), last)


def piece_of(stream, blocks, last):
    """The piece from what encode_slice gave for its slice."""
    if last:
        return stream[2:-4]
    bits = int.from_bytes(stream, "little")
    end = 16
    for start, end, eof in blocks:
        if eof:
            bits &= ~(1 << start)
    assert not blocks or blocks[-1][2], "a one-shot encode ends with a final block"
    bits &= (1 << end) - 1                      # (drops the Adler-32; the padding behind `end` is zero anyway)
    nbytes = (end + 3 + 7) // 8                 # three zero bits, padded to a byte
    return bits.to_bytes(nbytes, "little")[2:] + SYNC


def cuts(size, piece_bytes):
    """[(start, end)] of the pieces of an input of `size` bytes: the empty input is one empty piece."""
    return [(k, min(k + piece_bytes, size)) for k in range(0, size, piece_bytes)] or [(0, 0)]


def pieces_count(size, piece_bytes):
    return len(range(0, size, piece_bytes)) or 1


def compress_bound(size):
    return size + size // 2 + 1024


def pieces_bound(size, piece_bytes):
    return 2 + sum(compress_bound(e - s) for s, e in cuts(size, piece_bytes)) + 4


def stitch(pieces, data):
    return b"\x78\x01" + b"".join(pieces) + (zlib.adler32(data) & 0xFFFFFFFF).to_bytes(4, "big")


def compress(data, level, piece_bytes):
    """The stitched stream of `data`."""
    data = bytes(data)
    spans = cuts(len(data), piece_bytes)
    return stitch([piece(data[s:e], level, k == len(spans) - 1) for k, (s, e) in enumerate(spans)], data)


def adler_join(x, y):
    """(A, B, len mod 65521) of a run of bytes followed by another, from theirs: the rule of the plan kernel."""
    (a1, b1, n1), (a2, b2, n2) = x, y
    return (a1 + a2 - 1) % MOD, (b1 + b2 + n2 * (a1 - 1)) % MOD, (n1 + n2) % MOD


def adler_of_pieces(data, piece_bytes):
    """zlib.adler32 of `data`, combined in plain integers from the checksums of its pieces."""
    whole = (1, 0, 0)
    for s, e in cuts(len(data), piece_bytes):
        ad = zlib.adler32(data[s:e])
        whole = adler_join(whole, (ad & 0xFFFF, ad >> 16, (e - s) % MOD))
    return whole[1] << 16 | whole[0]


# ---- the pinned inputs: a non-last piece of more than one block ----

def words_input(nwords=20000, seed=23):
    """Six-byte words of a dictionary of 1 024 with one or two random bytes between them (149 878 bytes): a symbol
    every four bytes where the words are found, so that a block fills (16 384 symbols) well inside the input."""
    r = np.random.default_rng(seed)
    w = r.integers(0, 256, (1024, 6), dtype=np.uint8)
    pick = r.integers(0, 1024, nwords)
    gap = r.integers(0, 256, (nwords, 2), dtype=np.uint8)
    glen = r.integers(1, 3, nwords)
    bb = bytearray()
    for i in range(nwords):
        bb += w[pick[i]].tobytes() + gap[i, :glen[i]].tobytes()
    return bytes(bb)


def noise_input(n=120000):
    """Noise over three symbols: 120 000 bytes are streams.chain_inputs()[0]."""
    return bytes(np.random.default_rng(5).integers(0, 3, n, dtype=np.uint8))


# level -> (input, blocks the model writes for it): inputs whose non-last piece has more than one block.  Level 1 finds
# the noise's matches and none of the words'; the chain and lazy parsers fill a block with the words, but for level 4
# (min_match 5 and a short search), which needs 150 000 bytes of the noise.
TWO_BLOCK = {1: ("noise", 2), 3: ("words", 2), 4: ("noise150", 2), 6: ("words", 2), 9: ("words", 2)}


@functools.lru_cache(maxsize=None)
def two_block_input(name):
    return {"noise": noise_input, "noise150": lambda: noise_input(150000), "words": words_input}[name]()


@functools.lru_cache(maxsize=None)
def two_block_pieces(level):
    """(input, its non-last piece, its last piece, number of blocks) at `level`, computed once per process."""
    data = two_block_input(TWO_BLOCK[level][0])
    stream, blocks = encode_slice(data, level)
    return data, piece_of(stream, blocks, False), piece_of(stream, blocks, True), len(blocks)
