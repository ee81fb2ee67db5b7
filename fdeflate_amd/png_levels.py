"""PNG encode at a compression level, 0 .. 9 (the C ABI of include/fdeflate_hip_png_levels.h), reached as
fdeflate_amd.png_levels.X.

The PNG encoders of fdeflate_amd.api and fdeflate_amd.png16_encode end in the ultra-fast encoder and stay as they are.
The pipelines here put fdeflate_amd.levels.deflate_level_batch behind the same front: png_filter_mixed_batch chooses
every row's filter and writes the filtered rows to memory in one pass over the packed scanlines, the level encoder
writes each zlib stream straight behind its file's prefix, and api.png_frame_mixed_batch makes the files.  They are
mixed pipelines -- every picture has its own size and depth / colour pair -- and serve uniform batches as batches of
equal records; there are no per-geometry variants.  The calls go through api._call: the same device, dtype and stream
checks as every batched entry point, and no fallback where the library or the GPU is missing.
"""
from . import _lib, api, levels
from .api import PNG_BAD_SIZES, PNG_FILE_SUFFIX, _call, _i32
from .levels import _level

__all__ = ["PNG_FILTER_GIVEN_TYPES", "level_bound", "level_file_bound", "png_filter_mixed_batch",
           "png_encode_mixed_files_level_batch", "png_encode_mixed_rgba_files_level_batch",
           "png_encode_mixed_rgba16_files_level_batch"]

PNG_FILTER_GIVEN_TYPES = 1   # flags bit 0 of png_filter_mixed_batch: `types` is input


def level_bound(size, level):
    """The slot levels.deflate_level_batch needs for `size` bytes at `level` (fdh_png_level_bound): api.stored_size at
    level 0, api.compress_bound at 1 .. 9.  size: an int (-> int, the library's arithmetic) or an int64 tensor (-> a
    tensor on its device, the same arithmetic in torch, so that the pipelines size their slots without a read-back)."""
    level = _level(level)
    if isinstance(size, int):
        return int(_lib.lib().fdh_png_level_bound(size, level))
    import torch
    if level:
        return size + size // 2 + 1024
    blocks = size // 65535
    rest = size - blocks * 65535
    return 2 + blocks * (5 + 65535) + torch.where(rest != 0, rest + 5, torch.full_like(rest, 2)) + 4


def level_file_bound(rows, row_bytes, level, prefix=api.PNG_FILE_PREFIX):
    """The file slot of a picture of `rows` rows of `row_bytes` bytes at `level` whose zlib stream starts `prefix` bytes
    into the file (fdh_png_level_file_bound): prefix + level_bound(rows * (row_bytes + 1), level) + 16."""
    return int(_lib.lib().fdh_png_level_file_bound(int(rows), int(row_bytes), _level(level), int(prefix)))


def png_filter_mixed_batch(pix, pix_off, types, types_off, filt, filt_off, info, upstream=None, flags=0, png_status=None):
    """Filter selection and filtering in one pass, every picture at its own row_bytes and bpp (fdh_png_filter_mixed_batch):
    picture i's packed scanlines at pix[pix_off[i] .. pix_off[i+1]) go to filt[filt_off[i] .. filt_off[i+1]) as height rows
    of 1 + row_bytes bytes, the type byte first.  The slots must be exact.  flags 0: every row's type is chosen as
    api.png_choose_filters_mixed_batch chooses it and written to `types` (types and types_off may both be None);
    PNG_FILTER_GIVEN_TYPES: `types` is input.
    -> png_status: 0 ok, 1 a given type above 4, 2 the slots are not the plan's (nothing written), 3 not encodable, or
    upstream[i]; a picture with 2, 3 or upstream[i] has its filt slot zeroed where that has the size its record asks for."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_filter_mixed_batch", pix, pix_off, types, types_off, filt, filt_off, info, upstream, int(flags), png_status, n)
    return png_status


def _file_sizes(level, bound=None):
    """The default file slots of a plan at `level`: prefix + level_bound(filtered size) + 16, 0 where the plan failed.
    bound: the stream slot of a tensor of sizes where it is not level_bound's (fdeflate_amd.pieces)."""
    def sizes(pix_size, types_size, prefix, planned):
        import torch
        stream = bound(pix_size + types_size) if bound else level_bound(pix_size + types_size, level)
        size = prefix + stream + PNG_FILE_SUFFIX
        return torch.where(planned == 0, size, torch.zeros_like(size))
    return sizes


def _encoder_slots(file_off, prefix, status):
    """api._enc_off for the level encoder, which takes no upstream: a picture that has failed gets an EMPTY slot -- its
    offset is that of the next picture that has not, or the end -- so the encoder writes nothing for it (out_len -1) and
    its file slot stays as it was; the slot of the sound picture in front of it only grows."""
    import torch
    n = file_off.numel() - 1
    enc_off = api._enc_off(file_off, prefix)
    starts = torch.where(status != 0, torch.full_like(enc_off[:n], 1 << 62), enc_off[:n])
    starts = torch.minimum(starts, enc_off[n])
    enc_off[:n] = torch.flip(torch.cummin(torch.flip(starts, (0,)), 0).values, (0,))
    return enc_off


def _behind_the_pixels(pix, pix_off, types, types_off, filt_off, total_filt, info, status, level, file, file_off, prefix,
                       pal, colour, trns_len, encoder=None):
    """Steps 2 .. 5 of every pipeline here: the filtered rows, the level encoder behind each prefix, the framing.
    encoder: levels.deflate_level_batch, or a call with its first five parameters and its result (fdeflate_amd.pieces)."""
    import torch
    filt = torch.empty(max(1, total_filt), dtype=torch.uint8, device=pix.device)
    status = png_filter_mixed_batch(pix, pix_off, types, types_off, filt, filt_off, info, upstream=status,
                                    flags=PNG_FILTER_GIVEN_TYPES if types is not None else 0)
    idat_len = (encoder or levels.deflate_level_batch)(filt, filt_off, file, _encoder_slots(file_off, prefix, status), level)
    status = torch.where((status == 0) & (idat_len == -1), torch.full_like(status, PNG_BAD_SIZES), status)
    idat_len = torch.where(status != 0, torch.zeros_like(idat_len), idat_len)     # (the framing then writes nothing)
    file_len, framed = api.png_frame_mixed_batch(file, file_off, idat_len, info, pal, colour, trns_len)
    return file_len, api._first(status, framed)


def png_encode_mixed_files_level_batch(pix, pix_off, info, level, pal=None, colour=None, trns_len=None, upstream=None, types=None,
                                       types_off=None, file=None, file_off=None):
    """Packed scanlines in, PNG files at `level` out, on torch's current stream.  info: ENCODABLE records (int32 [n, 8],
    api.png_encode_records with pairs); picture i's scanlines are pix[pix_off[i] .. pix_off[i+1]), exactly height_i rows of
    its row_bytes.  pal / colour / trns_len: as api.png_analyse_mixed_batch writes them, needed for colour type 3.
    types / types_off: the rows' filter types (both or neither; by default they are chosen).  file / file_off: the
    caller's slots (both or neither); by default slot i is prefix_i + level_bound(height_i * (row_bytes_i + 1), level) + 16,
    which always suffices.  The steps: api.png_encode_plan_batch on a copy of the records, ONE read-back of 16 bytes (the
    totals of the filtered bytes and of the file slots), png_filter_mixed_batch, levels.deflate_level_batch straight behind
    each file's prefix (which reads back the two ends of its input offsets, as it always does), api.png_frame_mixed_batch.
    -> (file, file_off, file_len, png_status, info): png_status[i] the first that is not 0 of upstream, the plan (2, 3,
    10, 11), the filters (1, 2, 3), the encoder (2: the slot is too small) and the framing; a picture that fails gets
    file_len[i] = 0 and nothing is written to its slot.  ValueError for a level outside 0 .. 9, before any device work."""
    return _files_level_pipeline(pix, pix_off, info, level, pal, colour, trns_len, upstream, types, types_off, file, file_off)


def _files_level_pipeline(pix, pix_off, info, level, pal, colour, trns_len, upstream, types, types_off, file, file_off, bound=None,
                          encoder=None):
    """png_encode_mixed_files_level_batch, with the stream slots and the encoder of the caller where it names them."""
    import torch
    level = _level(level)
    n = pix_off.numel() - 1
    dev = pix.device
    if (file is None) != (file_off is None):
        raise ValueError("file and file_off go together")
    if (types is None) != (types_off is None):
        raise ValueError("types and types_off go together")
    if n == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return (file if file is not None else torch.empty(0, dtype=torch.uint8, device=dev),
                file_off if file_off is not None else torch.zeros(1, dtype=torch.int64, device=dev), e, e.clone(), info)
    # (a copy: the plan gives a dimension record a pair, and such a record is not this call's to take: the filters say 3)
    pix_size, types_size, prefix, _, planned = api.png_encode_plan_batch(info.clone(), colour, trns_len, file_size=False)
    if upstream is not None:
        planned = api._first(upstream, planned)
    filt_size = torch.where(planned == 0, pix_size + types_size, torch.zeros_like(pix_size))
    file_size = _file_sizes(level, bound)(pix_size, types_size, prefix, planned)
    offs = torch.zeros((2, n + 1), dtype=torch.int64, device=dev)
    torch.cumsum(torch.stack((filt_size, file_size)), 1, out=offs[:, 1:])
    total_filt, total_file = api._read_back(offs[:, n])                            # the one read-back: 16 bytes
    if file is None:
        file = torch.empty(max(1, total_file), dtype=torch.uint8, device=dev)
        file_off = offs[1]
    else:
        slot = file_off[1:] - file_off[:-1]
        planned = torch.where((planned == 0) & (slot < prefix + PNG_FILE_SUFFIX), torch.full_like(planned, PNG_BAD_SIZES), planned)
        prefix = torch.minimum(prefix, slot)
    file_len, status = _behind_the_pixels(pix, pix_off, types, types_off, offs[0], total_filt, info, planned, level, file, file_off,
                                          prefix, pal, colour, trns_len, encoder)
    return file, file_off, file_len, status, info


def _rgba_level_pipeline(pictures, pictures_off, width, height, level, allowed, pairs, file, file_off, analyse, plan, pack,
                         bound=None, encoder=None):
    level = _level(level)
    front = api._png_encode_mixed_front(pictures, pictures_off, width, height, allowed, pairs, file, file_off, analyse, plan, pack,
                                        file_size=_file_sizes(level, bound))
    if len(front) == 5:
        return front
    pix, offs, total_types, file, file_off, prefix, status, info, pal, colour, trns_len = front
    # the filtered rows: a type byte per row more than the packed scanlines, so the offsets and the total follow from
    # the front's sums without another read-back (no rows: no pixels, and `pix` is one spare byte)
    filt_off = offs[0] + offs[1]
    total_filt = pix.numel() + total_types if total_types else 0
    file_len, status = _behind_the_pixels(pix, offs[0], None, None, filt_off, total_filt, info, status, level, file, file_off, prefix,
                                          pal, colour, trns_len, encoder)
    return file, file_off, file_len, status, info


def png_encode_mixed_rgba_files_level_batch(rgba, rgba_off, width, height, level, allowed=0, pairs=None, file=None, file_off=None):
    """api.png_encode_mixed_rgba_files_batch at a compression level: the same arguments and results, and `level`, 0 .. 9
    (ValueError for anything else, before any device work).  The front is that call's own -- analysis, plan, the ONE
    read-back of 24 bytes, packing; the totals of the filtered rows follow from those three, so no further read-back is
    made here (levels.deflate_level_batch reads back the two ends of its input offsets, as it always does) -- then
    png_filter_mixed_batch into exact slots (size 0 for a picture whose plan failed), levels.deflate_level_batch straight
    behind each file's prefix, out_len -1 as status 2, api.png_frame_mixed_batch.  The default file slot of picture i is
    prefix_i + level_bound(height_i * (row_bytes_i + 1), level) + 16; a caller's slot shorter than prefix_i + 16, or too
    small for the stream, is status 2 and file_len 0.  Nothing is written to the slot of a picture that fails.
    -> (file, file_off, file_len, png_status, info)."""
    return _rgba_level_pipeline(rgba, rgba_off, width, height, level, allowed, pairs, file, file_off, api.png_analyse_mixed_batch,
                                api.png_encode_plan_batch, api.png_pack_mixed_batch)


def png_encode_mixed_rgba16_files_level_batch(rgba16, rgba16_off, width, height, level, allowed=0, pairs=None, file=None,
                                              file_off=None):
    """png16_encode.png_encode_mixed_rgba16_files_batch at a compression level: png_encode_mixed_rgba_files_level_batch
    with that call's front (png_analyse16_mixed_batch, png_encode16_plan_batch, png_pack16_mixed_batch).  A picture whose
    samples are all narrow gets the file, byte for byte, that png_encode_mixed_rgba_files_level_batch makes of its high
    bytes at the same level.  -> (file, file_off, file_len, png_status, info);
    png16.png_decode_mixed_files_rgba16_batch gives the pictures back."""
    from . import png16_encode as e16
    return _rgba_level_pipeline(rgba16, rgba16_off, width, height, level, allowed, pairs, file, file_off, e16.png_analyse16_mixed_batch,
                                e16.png_encode16_plan_batch, e16.png_pack16_mixed_batch)
