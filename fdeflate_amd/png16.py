"""PNG decode and encode at 16 bits per sample (the C ABI of include/fdeflate_hip_png16.h), reached as
fdeflate_amd.png16.X.

An RGBA16 picture is [H, W, 4] samples of 16 bits in R, G, B, A order, each in the device's own (little-endian) byte
order.  Buffers are uint8 tensors with int64 byte offsets like every other buffer of the package:
rgba16[rgba16_off[i]:rgba16_off[i+1]].view(torch.uint16) -- or .view(torch.int16) -- .view(h, width, 4) is picture i.
The calls go through api._call: the same device, dtype and stream checks as every batched entry point, and no
fallback where the library or the GPU is missing.
"""
from . import api
from .api import PNG_FILE_PREFIX, _call, _i32

__all__ = ["png_expand16_batch", "png_expand16_mixed_batch", "png_pack16_batch", "png_decode_files_rgba16_batch",
           "png_decode_mixed_files_rgba16_batch", "png_encode_rgba16_files_batch"]


def png_expand16_batch(pix, pix_off, rgba16, rgba16_off, width, bit_depth, colour_type, pal=None, colour=None, upstream=None,
                       png_status=None):
    """Packed scanlines to RGBA16 (fdh_png_expand16_batch): image i, whole rows at pix_off[i] .. pix_off[i+1], goes to the
    slot rgba16[rgba16_off[i] .. rgba16_off[i+1]) of exactly rows * width * 8 bytes, which must start at an even address;
    samples are in the device's byte order and scaled exactly (depth 16 as it is, depth 8 * 257, 4 * 4369, 2 * 21845,
    1 * 65535; palette entries and their alphas * 257; the key compared on the raw samples, alpha 0 or 65535).  pal /
    colour as api.png_colour_batch writes them (pal is needed for colour type 3; without colour there is no key and
    every palette index counts as inside); upstream (int32 [n]): where not 0 the image is skipped and its png_status is
    that value.  -> png_status: 0 ok, 2 the slots do not fit or the output slot is misaligned (nothing written),
    PNG_INDEX_OUTSIDE_PALETTE (9: such pixels are (0, 0, 0, 65535))."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_expand16_batch", pix, pix_off, rgba16, rgba16_off, pal, colour, upstream, png_status, n, width, bit_depth,
          colour_type)
    return png_status


def png_expand16_mixed_batch(pix, pix_off, rgba16, rgba16_off, info, pal=None, colour=None, upstream=None, png_status=None):
    """png_expand16_batch at every image's own geometry (fdh_png_expand16_mixed_batch).  pal / colour as
    api.png_colour_mixed_batch writes them; an image of colour type 3 without `pal` is status 10.
    -> png_status: 0 ok, 2 the slots do not fit or the output slot is misaligned, 3 not decodable, 9 an index outside
    the palette, or upstream[i]."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_expand16_mixed_batch", pix, pix_off, rgba16, rgba16_off, info, pal, colour, upstream, png_status, n)
    return png_status


def png_pack16_batch(rgba16, rgba16_off, pix, pix_off, width, colour_type, upstream=None, png_status=None):
    """RGBA16 to packed scanlines of depth 16, the inverse of png_expand16_batch for colour types 0, 2, 4 and 6
    (fdh_png_pack16_batch): image i, whole rows of width * 8 bytes at rgba16_off[i] .. rgba16_off[i+1] (an even address),
    goes to the slot pix[pix_off[i] .. pix_off[i+1]) of exactly rows * row_bytes bytes, samples big-endian.  No colour
    key is written.  upstream (int32 [n]): where not 0 the image is skipped and its png_status is that value.
    -> png_status: 0 ok, 2 the slots do not fit or the RGBA16 slot is misaligned (nothing written),
    PNG_NOT_REPRESENTABLE (13: colour type 0 or 4 and R, G, B not all equal, or colour type 0 or 2 and A != 65535; the
    slot's contents are then not specified).  Colour type 3 or any other value raises."""
    n = rgba16_off.numel() - 1
    png_status = _i32(png_status, rgba16, n)
    _call("fdh_png_pack16_batch", rgba16, rgba16_off, pix, pix_off, upstream, png_status, n, width, colour_type)
    return png_status


def png_decode_files_rgba16_batch(file, file_off, width, bit_depth, colour_type, file_len=None, flags=0):
    """PNG files in, RGBA16 pictures out, on torch's current stream: api.png_decode_files_rgba_batch's steps (the same
    single read-back of `info`, which also sizes the RGBA16 slots: height * width * 8 bytes, empty for files that are
    skipped) with png_expand16_batch at the end; `flags` as there (PNG_FLAG_ADAM7 included).
    -> (rgba16, rgba16_off, info, status, png_status):
    rgba16[rgba16_off[i]:rgba16_off[i+1]].view(torch.uint16).view(h, width, 4) is picture i -- samples of depth 16 as
    they are, in the device's byte order, lower depths scaled exactly, palette and tRNS applied (PNG specification; no
    gamma) --; info and status as api.png_decode_files_batch; png_status the first that is not 0 of gather, colour,
    inflate_png_batch and expand (3, 7; 10, 11; 1 .. 3; 9)."""
    decoded = api._png_files_to_pixels(file, file_off, width, bit_depth, colour_type, file_len, flags, True)
    return api._png_pixels_to_rgba(decoded, 2, png_expand16_batch, png_expand16_mixed_batch)


def png_decode_mixed_files_rgba16_batch(file, file_off, file_len=None, flags=0, max_bytes=0, route=None):
    """api.png_decode_mixed_files_rgba_batch to RGBA16: the same steps, the same ONE read-back of 48 bytes and the same
    route selection, with png_expand16_mixed_batch (or png_expand16_batch on the uniform route) at the end.  max_bytes:
    as there, and a file whose RGBA16 picture (height * width * 8 bytes) would be larger is png_status 2 with empty
    slots as well.
    -> (rgba16, rgba16_off, info, status, png_status): rgba16[rgba16_off[i]:rgba16_off[i+1]].view(torch.uint16)
    .view(height_i, width_i, 4) is picture i as png_decode_files_rgba16_batch makes it; png_status the first that is not
    0 of plan, gather, colour, reconstruction and expansion (2, 3; 3, 8; 10, 11; 1 .. 3; 9)."""
    decoded = api._png_mixed_files_to_pixels(file, file_off, file_len, flags, max_bytes, route, True, sample_bytes=2)
    return api._png_pixels_to_rgba(decoded, 2, png_expand16_batch, png_expand16_mixed_batch)


def png_encode_rgba16_files_batch(rgba16, rgba16_off, file, file_off, width, colour_type):
    """RGBA16 pictures in, PNG files of depth 16 and the given colour type (0, 2, 4 or 6) out, on torch's current stream
    and without a read-back: png_pack16_batch, the rows' filter types and the fused filter + ultra-fast encode
    (api.png_encode_ultrafast_batch) at file_off + 41, and api.png_frame_batch around the streams.  Image i is
    rgba16[rgba16_off[i] .. rgba16_off[i+1]), whole rows of width * 8 bytes in the device's byte order; its file goes to
    the slot file[file_off[i] .. file_off[i+1]) -- api.png_file_bound(rows, row_bytes) always suffices.
    -> (file_len, png_status): png_status[i] is the first that is not 0 of pack (2, 13), the encoder and the framing (2);
    an image that failed in front of the framing gets no file: file_len[i] = 0, nothing is framed, and the contents of
    its file slot are not specified.
    The encoders take ONE offsets array, so the encoder's slot for image i reaches 41 bytes into slot i + 1 (the last
    one ends 16 bytes in front of its slot's end): the bytes that image i + 1's own prefix is written to afterwards.  A
    stream that does not fit its file slot can therefore leave bytes in the first 41 of the next slot; they stay there
    only if that next image fails as well."""
    if colour_type not in (0, 2, 4, 6):
        raise ValueError("colour_type must be 0, 2, 4 or 6 (the pairs of depth 16)")
    row_bytes, bpp = api.png_geometry(width, 16, colour_type)
    return api._png_rgba_to_files(
        rgba16, rgba16_off, file, file_off, width, 8, row_bytes, bpp, PNG_FILE_PREFIX,
        lambda pix, pix_off: png_pack16_batch(rgba16, rgba16_off, pix, pix_off, width, colour_type),
        lambda idat_len, height: api.png_frame_batch(file, file_off, idat_len, height, width, 16, colour_type))
