"""Long inputs encoded in parallel pieces at levels 1 .. 9, PNG files included (the C ABI of
include/fdeflate_hip_pieces.h), reached as fdeflate_amd.pieces.X.

fdeflate_amd.levels.deflate_level_batch encodes one stream per lane of its parser and per wavefront of its block writer,
which suits thousands of short streams and leaves the device idle on one long one.  The calls here cut every input at
multiples of `piece_bytes`, encode the pieces as independent raw-deflate streams with the same kernels (the non-last
ones closed on a byte boundary by the sync marker 00 00 FF FF), and stitch them into one zlib stream per input:
78 01, the pieces, the Adler-32 of the whole input, combined from the pieces' on the device.  An input of at most
piece_bytes bytes is one piece and gives levels.deflate_level_batch's stream byte for byte; a longer one gives a stream
that is a little larger (a piece cannot refer to the bytes in front of it) and inflates to the same bytes.  Opt-in:
nothing else in the package calls this module.  Level 0 has no piece mode -- stored blocks are copied in parallel as it
is -- and goes down the existing route.  No fallback where the library or the GPU is missing.
"""
from . import _lib, api, levels, png_levels
from .api import _call, _i32
from .levels import _level

__all__ = ["PIECE_BYTES_DEFAULT", "PIECE_BYTES_MIN", "PIECE_BYTES_MAX", "pieces_count", "pieces_bound", "pieces_file_bound",
           "deflate_level_pieces_raw_batch", "deflate_stitch_batch", "deflate_level_pieces_batch", "compress_to_vec_level_pieces",
           "png_encode_mixed_files_level_pieces_batch", "png_encode_mixed_rgba_files_level_pieces_batch",
           "png_encode_mixed_rgba16_files_level_pieces_batch"]

PIECE_BYTES_DEFAULT = 65536     # the stream size every encoder figure of the README was measured at; twice the window
PIECE_BYTES_MIN = 64
PIECE_BYTES_MAX = 1 << 30


def _piece_bytes(piece_bytes):
    if isinstance(piece_bytes, bool) or not isinstance(piece_bytes, int) or not PIECE_BYTES_MIN <= piece_bytes <= PIECE_BYTES_MAX:
        raise ValueError("piece_bytes %r is outside %d .. 2^30" % (piece_bytes, PIECE_BYTES_MIN))
    return piece_bytes


def pieces_count(size, piece_bytes=PIECE_BYTES_DEFAULT):
    """The pieces of an input of `size` bytes: max(1, ceil(size / piece_bytes)) (fdh_deflate_pieces_count).  size: an int
    (the library's arithmetic) or an int64 tensor (the same in torch, on its device)."""
    piece_bytes = _piece_bytes(piece_bytes)
    if isinstance(size, int):
        return int(_lib.lib().fdh_deflate_pieces_count(size, piece_bytes))
    return ((size + (piece_bytes - 1)) // piece_bytes).clamp(min=1)


def pieces_bound(size, level, piece_bytes=PIECE_BYTES_DEFAULT):
    """The slot deflate_level_pieces_batch needs for `size` bytes at `level` (fdh_deflate_pieces_bound): 2 + the sum of
    api.compress_bound over the pieces + 4 at levels 1 .. 9, api.stored_size at level 0, where the input goes to
    levels.deflate_level_batch.  size: an int or an int64 tensor, as for pieces_count."""
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    if isinstance(size, int):
        return int(_lib.lib().fdh_deflate_pieces_bound(size, level, piece_bytes))
    if level == 0:
        return png_levels.level_bound(size, 0)
    full = size // piece_bytes
    rest = size - full * piece_bytes
    one = (rest != 0) | (full == 0)
    return 2 + full * api.compress_bound(piece_bytes) + one * (rest + rest // 2 + 1024) + 4


def pieces_file_bound(rows, row_bytes, level, piece_bytes=PIECE_BYTES_DEFAULT, prefix=api.PNG_FILE_PREFIX):
    """png_levels.level_file_bound for the piece pipelines (fdh_png_level_pieces_file_bound): prefix +
    pieces_bound(rows * (row_bytes + 1), level, piece_bytes) + 16."""
    return int(_lib.lib().fdh_png_level_pieces_file_bound(int(rows), int(row_bytes), _level(level), _piece_bytes(piece_bytes), int(prefix)))


def _piece_level(level):
    if _level(level) == 0:
        raise ValueError("level 0 has no piece mode (levels 1 .. 9 have)")
    return level


def deflate_level_pieces_raw_batch(raw, piece_off, piece_last, out, out_off, level, out_len=None, piece_adler=None):
    """levels.deflate_level_batch in piece mode (fdh_deflate_level_pieces_batch): piece k is raw[piece_off[k] ..
    piece_off[k+1]), encoded as raw deflate into out[out_off[k] .. out_off[k+1]); piece_last (uint8) is not 0 for the last
    piece of its input, which gets BFINAL and the padding, every other piece ends with the sync marker.  Slots of
    api.compress_bound(piece length) always suffice.  -> (out_len, piece_adler): the pieces' lengths (-1: the slot is too
    small) and the Adler-32 of their bytes.  Levels 1 .. 9.  Returns when the work has finished."""
    level = _piece_level(level)
    n = piece_off.numel() - 1
    out_len, piece_adler = _i32(out_len, raw, n), _i32(piece_adler, raw, n)
    _call("fdh_deflate_level_pieces_batch", raw, piece_off, piece_last, out, out_off, out_len, piece_adler, n, level)
    return out_len, piece_adler


def deflate_stitch_batch(pieces, piece_slot_off, piece_len, piece_adler, piece_off, first_piece, out, out_off, out_len=None):
    """Joins pieces into zlib streams (fdh_deflate_stitch_batch): input i owns the pieces first_piece[i] ..
    first_piece[i+1], piece k lies at pieces[piece_slot_off[k] ..) with piece_len[k] bytes, covers the raw bytes
    piece_off[k] .. piece_off[k+1] and has the checksum piece_adler[k].  out[out_off[i] ..) receives 78 01, the pieces
    and the combined Adler-32; out_len[i] = -1 where a piece has failed or the stream does not fit, and nothing is
    written there.  piece_adler is overwritten (with every piece's position in its stream).  `pieces` and `out` must not
    overlap.  Enqueued on torch's current stream; no host synchronisation."""
    n = first_piece.numel() - 1
    out_len = _i32(out_len, out, n)
    _call("fdh_deflate_stitch_batch", pieces, piece_slot_off, piece_len, piece_adler, piece_off, first_piece, out, out_off, out_len, n)
    return out_len


def deflate_level_pieces_batch(raw, in_off, out, out_off, level, piece_bytes=PIECE_BYTES_DEFAULT, out_len=None):
    """levels.deflate_level_batch with every input cut into pieces of piece_bytes: the same arguments and result, the
    streams as the module's text describes them.  Slots of pieces_bound(len_i, level, piece_bytes) always suffice;
    out_len[i] = -1 for a slot that is too small.  The inputs must lie in `raw` in order (in_off ascending), as every
    caller here has them.  The piece table -- offsets, last flags, each input's range -- is made on the device; ONE
    read-back of 8 bytes, the number of pieces, sizes the launches and the scratch of the pieces' slots (1.5 x
    raw.numel() + 1 040 per piece), and the encoder reads back the two ends of its offsets as
    levels.deflate_level_batch does.  Level 0: levels.deflate_level_batch itself."""
    import torch
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    if level == 0:
        return levels.deflate_level_batch(raw, in_off, out, out_off, 0, out_len)
    n = in_off.numel() - 1
    out_len = _i32(out_len, raw, n)
    if n == 0:
        return out_len
    dev = raw.device
    size = in_off[1:] - in_off[:-1]
    count = pieces_count(size, piece_bytes)
    first_piece = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=first_piece[1:])
    total, = api._read_back(first_piece[n:])                                       # the one read-back: 8 bytes
    owner = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), count, output_size=total)
    index = torch.arange(total, dtype=torch.int64, device=dev) - first_piece[owner]
    piece_off = torch.empty(total + 1, dtype=torch.int64, device=dev)
    torch.add(in_off[owner], index * piece_bytes, out=piece_off[:total])
    piece_off[total] = in_off[n]
    piece_last = (index == count[owner] - 1).to(torch.uint8)
    # a slot of compress_bound per piece, on a 16-byte boundary (the block writer stores lines of 16 bytes)
    piece_size = piece_off[1:] - piece_off[:-1]
    slot_off = torch.zeros(total + 1, dtype=torch.int64, device=dev)
    torch.cumsum((piece_size + piece_size // 2 + (1024 + 15)) & ~15, 0, out=slot_off[1:])
    slots = torch.empty(raw.numel() + raw.numel() // 2 + 1040 * total, dtype=torch.uint8, device=dev)
    piece_len, piece_adler = deflate_level_pieces_raw_batch(raw, piece_off, piece_last, slots, slot_off, level)
    return deflate_stitch_batch(slots, slot_off, piece_len, piece_adler, piece_off, first_piece, out, out_off, out_len)


def compress_to_vec_level_pieces(data, level, piece_bytes=PIECE_BYTES_DEFAULT):
    """levels.compress_to_vec_with_level through deflate_level_pieces_batch: host bytes in, the stitched zlib stream as
    bytes out.  ValueError for a level outside 0 .. 9 or a piece_bytes outside 64 .. 2^30, before any device work."""
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    data = bytes(data)
    if _lib.lib().fdh_device_count() <= 0:
        raise _lib.FdeflateHipError("no HIP device: fdeflate_hip has no CPU fallback")
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    raw = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).to(dev)
    bound = pieces_bound(len(data), level, piece_bytes)
    in_off = torch.tensor([0, len(data)], dtype=torch.int64, device=dev)
    out_off = torch.tensor([0, bound], dtype=torch.int64, device=dev)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    got = int(deflate_level_pieces_batch(raw, in_off, out, out_off, level, piece_bytes)[0])
    if got < 0:
        raise _lib.FdeflateHipError("internal: encoder bound exceeded")
    return out[:got].cpu().numpy().tobytes()


def _routes(level, piece_bytes):
    """(bound, encoder) as png_levels' pipelines take them: the stitched slot of a tensor of sizes, and
    deflate_level_pieces_batch at this piece size."""
    def encoder(raw, in_off, out, out_off, level):
        return deflate_level_pieces_batch(raw, in_off, out, out_off, level, piece_bytes)
    return (lambda size: pieces_bound(size, level, piece_bytes)), encoder


def png_encode_mixed_files_level_pieces_batch(pix, pix_off, info, level, pal=None, colour=None, trns_len=None, upstream=None, types=None,
                                              types_off=None, file=None, file_off=None, piece_bytes=PIECE_BYTES_DEFAULT):
    """png_levels.png_encode_mixed_files_level_batch with every picture's filtered rows encoded in pieces of piece_bytes:
    the same arguments, steps and results, with deflate_level_pieces_batch (one more read-back, of 8 bytes) where that
    has levels.deflate_level_batch.  The default file slot of picture i is prefix_i + pieces_bound(height_i *
    (row_bytes_i + 1), level, piece_bytes) + 16.  A picture whose filtered rows are at most piece_bytes gets that call's
    file byte for byte; a picture that fails keeps file_len 0 and an untouched slot."""
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    return png_levels._files_level_pipeline(pix, pix_off, info, level, pal, colour, trns_len, upstream, types, types_off, file, file_off,
                                            *_routes(level, piece_bytes))


def png_encode_mixed_rgba_files_level_pieces_batch(rgba, rgba_off, width, height, level, allowed=0, pairs=None, file=None, file_off=None,
                                                   piece_bytes=PIECE_BYTES_DEFAULT):
    """png_levels.png_encode_mixed_rgba_files_level_batch in pieces: as png_encode_mixed_files_level_pieces_batch is to
    its namesake.  -> (file, file_off, file_len, png_status, info)."""
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    return png_levels._rgba_level_pipeline(rgba, rgba_off, width, height, level, allowed, pairs, file, file_off,
                                           api.png_analyse_mixed_batch, api.png_encode_plan_batch, api.png_pack_mixed_batch,
                                           *_routes(level, piece_bytes))


def png_encode_mixed_rgba16_files_level_pieces_batch(rgba16, rgba16_off, width, height, level, allowed=0, pairs=None, file=None,
                                                     file_off=None, piece_bytes=PIECE_BYTES_DEFAULT):
    """png_levels.png_encode_mixed_rgba16_files_level_batch in pieces: as png_encode_mixed_files_level_pieces_batch is to
    its namesake.  -> (file, file_off, file_len, png_status, info)."""
    from . import png16_encode as e16
    level, piece_bytes = _level(level), _piece_bytes(piece_bytes)
    return png_levels._rgba_level_pipeline(rgba16, rgba16_off, width, height, level, allowed, pairs, file, file_off,
                                           e16.png_analyse16_mixed_batch, e16.png_encode16_plan_batch, e16.png_pack16_mixed_batch,
                                           *_routes(level, piece_bytes))
