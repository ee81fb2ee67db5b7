"""PNG encode of mixed batches of RGBA16 pictures, the depth / colour pair chosen per picture (the C ABI of
include/fdeflate_hip_png16_encode.h), reached as fdeflate_amd.png16_encode.X.

An RGBA16 picture is what fdeflate_amd.png16 describes: [H, W, 4] samples of 16 bits in the device's byte order, in a
uint8 buffer with int64 byte offsets, its slot exactly height * width * 8 bytes at an even address.  A sample is narrow
when its two bytes are equal (s == 257 * (s >> 8)); a picture whose samples are all narrow is written as the RGBA8
picture of its high bytes would be.  The calls go through api._call: the same device, dtype and stream checks as every
batched entry point, and no fallback where the library or the GPU is missing.
"""
import ctypes as C

from . import _lib, api
from .api import PNG_INFO_WORDS, _call, _i32

__all__ = ["png_analyse16_mixed_batch", "png_encode16_plan_one", "png_encode16_plan_batch", "png_pack16_mixed_batch",
           "png_encode_mixed_rgba16_files_batch"]

PNG_SUMMARY_NARROW = 4   # summary bit 2: every sample is narrow (bits 0 and 1: api.PNG_SUMMARY_OPAQUE, api.PNG_SUMMARY_GREY)


def png_analyse16_mixed_batch(rgba16, rgba16_off, info, max_colours=256, with_pal=True, upstream=None, pal=None, colour=None,
                              trns_len=None, summary=None, png_status=None):
    """What every RGBA16 picture is (fdh_png_analyse16_mixed_batch): the slot of image i must be exactly
    height_i * width_i * 8 bytes at an even address.  info: dimension records or encodable ones (api.png_encode_records).
    -> (pal, colour, trns_len, summary, png_status).  summary: bit 0 every A is 65535, bit 1 R == G == B on all 16 bits,
    bit 2 every sample is narrow, bits 8 .. 15 the smallest depth of 1, 2, 4, 8, 16 that holds every R, G, B.  Where bit 2
    is set, pal / colour / trns_len are api.png_analyse_mixed_batch's for the picture of the high bytes.  png_status: 0,
    2 the slot does not fit or is misaligned (nothing written), 3 neither kind of record, 12 bit 2 is clear or more than
    max_colours distinct pixels (the summary is valid), or upstream[i] where that is not 0."""
    n = rgba16_off.numel() - 1
    if with_pal:
        pal = _i32(pal, rgba16, n, 256)
    colour, trns_len = _i32(colour, rgba16, n, 4), _i32(trns_len, rgba16, n)
    summary, png_status = _i32(summary, rgba16, n), _i32(png_status, rgba16, n)
    _call("fdh_png_analyse16_mixed_batch", rgba16, rgba16_off, info, upstream, pal, colour, trns_len, summary, png_status, n,
          max_colours)
    return pal, colour, trns_len, summary, png_status


def png_encode16_plan_one(record, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    """The encode plan of one RGBA16 picture (fdh_png_encode16_plan_one: host arithmetic, no device call); the parameters
    and the result are api.png_encode_plan_one's, summary and analyse_status png_analyse16_mixed_batch's.  An encodable
    record keeps its pair; a dimension record gets the pair of its high bytes' RGBA8 picture where summary bit 2 is set,
    and else the cheapest of (16, 0), (16, 4), (16, 2), (16, 6) that holds it (analyse_status 12 is no error then).
    -> (status, bit_depth, colour_type, packed, types, prefix, file)."""
    rec = api._PngInfoRecord(**{k: int(record.get(k, 0)) for k, _ in api._PngInfoRecord._fields_})
    have = count is not None and trns_len is not None
    c, t = C.c_uint32(int(count) if have else 0), C.c_uint32(int(trns_len) if have else 0)
    sizes = (C.c_uint64 * 4)()
    st = _lib.lib().fdh_png_encode16_plan_one(C.byref(rec), C.byref(c) if have else None, C.byref(t) if have else None, int(summary),
                                              int(analyse_status), int(allowed), sizes)
    return (int(st), int(rec.bit_depth), int(rec.colour_type)) + tuple(int(v) for v in sizes)


def png_encode16_plan_batch(info, colour=None, trns_len=None, summary=None, analyse_status=None, allowed=0, pix_size=True,
                            types_size=True, prefix=True, file_size=True, png_status=None):
    """png_encode16_plan_one for n records on the device (fdh_png_encode16_plan_batch); `info` is changed in place: a
    dimension record gets its pair.  colour / trns_len / summary / analyse_status as png_analyse16_mixed_batch writes them.
    The four outputs as in api.png_encode_plan_batch.
    -> (pix_size, types_size, prefix, file_size, png_status), None for an output that was not wanted."""
    n = info.numel() // PNG_INFO_WORDS
    outs = api._wanted(info, n, pix_size, types_size, prefix, file_size)
    png_status = _i32(png_status, info, n)
    _call("fdh_png_encode16_plan_batch", info, colour, trns_len, summary, analyse_status, int(allowed), *outs, png_status, n)
    return (*outs, png_status)


def png_pack16_mixed_batch(rgba16, rgba16_off, pix, pix_off, info, pal=None, colour=None, upstream=None, png_status=None):
    """RGBA16 pictures to the packed scanlines of every picture's own pair and width, all fifteen pairs
    (fdh_png_pack16_mixed_batch): the slots must be exactly height * width * 8 bytes (at an even address) and the plan's
    packed size.  Depth 16: png16.png_pack16_batch's bytes.  Depth 8 and below: every sample must be narrow, and the bytes
    are api.png_pack_batch's for the picture of the high bytes with the same pal / colour.
    -> png_status: 0 ok, 2 the slots do not fit, 3 not encodable, 10 colour type 3 without `pal`, 13 not representable
    (a sample that is not narrow included), or upstream[i]."""
    n = rgba16_off.numel() - 1
    png_status = _i32(png_status, rgba16, n)
    _call("fdh_png_pack16_mixed_batch", rgba16, rgba16_off, pix, pix_off, info, pal, colour, upstream, png_status, n)
    return png_status


def png_encode_mixed_rgba16_files_batch(rgba16, rgba16_off, width, height, allowed=0, pairs=None, file=None, file_off=None):
    """RGBA16 pictures of any size in, PNG files out, each with the smallest of the fifteen depth / colour pairs that holds
    it without loss (or with the pair `pairs` names, see api.png_encode_records), on torch's current stream:
    api.png_encode_mixed_rgba_files_batch's steps with the three RGBA16 calls in front -- png_analyse16_mixed_batch,
    png_encode16_plan_batch, the same ONE read-back of 24 bytes, png_pack16_mixed_batch -- and behind them
    api.png_choose_filters_mixed_batch, api.png_filter_deflate_ultrafast_mixed_batch and api.png_frame_mixed_batch.
    Picture i is rgba16[rgba16_off[i] .. rgba16_off[i+1]), exactly height[i] * width[i] * 8 bytes at an even address.
    allowed, file / file_off and the encoder's slots: as there.  A picture whose samples are all narrow gets the file,
    byte for byte, that api.png_encode_mixed_rgba_files_batch makes of its high bytes.
    -> (file, file_off, file_len, png_status, info) as there; png16.png_decode_mixed_files_rgba16_batch gives the pictures
    back."""
    import torch
    front = api._png_encode_mixed_front(rgba16, rgba16_off, width, height, allowed, pairs, file, file_off, png_analyse16_mixed_batch,
                                        png_encode16_plan_batch, png_pack16_mixed_batch)
    if len(front) == 5:
        return front
    pix, offs, total_types, file, file_off, prefix, status, info, pal, colour, trns_len = front
    types = torch.empty(max(1, total_types), dtype=torch.uint8, device=rgba16.device)
    status = api.png_choose_filters_mixed_batch(pix, offs[0], types, offs[1], info, upstream=status)
    enc_off = api._enc_off(file_off, prefix)
    idat_len, status = api.png_filter_deflate_ultrafast_mixed_batch(pix, offs[0], types, offs[1], file, enc_off, info, upstream=status)
    idat_len = torch.where(status != 0, torch.zeros_like(idat_len), idat_len)     # (the framing then writes nothing)
    file_len, framed = api.png_frame_mixed_batch(file, file_off, idat_len, info, pal, colour, trns_len)
    return file, file_off, file_len, api._first(status, framed), info
