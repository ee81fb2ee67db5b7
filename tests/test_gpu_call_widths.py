"""-m gpu: api._call holds every tensor to the element width that _lib.SIGNATURES records for its parameter.

A tensor of another width used to go to the kernel as a pointer: wrong results, or reads and writes past its end.
Now it is a ValueError that names the symbol, raised behind the device / contiguity checks (whose messages stay) and
in front of the launch: the outputs still hold their fill afterwards.  The same calls, well-typed, give what they gave
before.  n = 1 and a few bytes throughout.
"""
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
EMPTY_ZLIB = bytes((0x78, 0x01, 0x03, 0x00, 0x00, 0x00, 0x00, 0x01))


def _t(values, dtype):
    import torch
    return torch.tensor(list(values), dtype=dtype, device="cuda")


def _inflate():
    import torch
    import fdeflate_amd as fd
    args = dict(comp=_t(EMPTY_ZLIB, torch.uint8), in_off=_t((0, 8), torch.int64), out=_t((0,) * 4, torch.uint8),
                out_off=_t((0, 4), torch.int64), out_len=_t((FILL,), torch.int32), status=_t((FILL,), torch.int32),
                adler=_t((FILL,), torch.int32))
    return "fdh_inflate_batch", fd.inflate_batch, args, ("in_off", "status", "comp"), ("out_len", "status", "adler")


def _expand():
    import torch
    import fdeflate_amd as fd
    info = _t(((0, 1, 1, 8, 0, 0, 0, 0),), torch.int32)    # one grey-8 pixel
    args = dict(pix=_t((0x42,), torch.uint8), pix_off=_t((0, 1), torch.int64), rgba=_t((0,) * 4, torch.uint8),
                rgba_off=_t((0, 4), torch.int64), info=info, png_status=_t((FILL,), torch.int32))
    return "fdh_png_expand_mixed_batch", fd.png_expand_mixed_batch, args, ("rgba_off", "png_status", "rgba"), ("png_status",)


def _crc():
    import torch
    import fdeflate_amd as fd
    args = dict(data=_t(b"abc", torch.uint8), off=_t((0, 3), torch.int64), crc=_t((FILL,), torch.int32),
                status=_t((FILL,), torch.int32))
    return "fdh_crc32_batch", fd.crc32_batch, args, ("off", "crc", "data"), ("crc", "status")


CALLS = {"inflate_batch": _inflate, "png_expand_mixed_batch": _expand, "crc32_batch": _crc}


@pytest.mark.parametrize("which", sorted(CALLS))
def test_a_tensor_of_the_wrong_width_is_refused_before_the_launch(which):
    import torch
    symbol, call, args, (offsets, output, buffer), outputs = CALLS[which]()
    assert args[offsets].dtype == torch.int64 and args[output].dtype == torch.int32 and args[buffer].dtype == torch.uint8
    for name, dtype in ((offsets, torch.int32), (output, torch.int64), (buffer, torch.int32), (output, torch.float32)):
        wrong = dict(args)
        wrong[name] = args[name].to(dtype)
        with pytest.raises(ValueError, match=symbol + ": parameter"):
            call(**wrong)
    # the older checks come first and keep their words, whatever the width
    host = dict(args)
    host[offsets] = args[offsets].to(torch.int32).cpu()
    with pytest.raises(ValueError, match="batched entry points take device tensors"):
        call(**host)
    strided = dict(args)
    strided[buffer] = args[buffer].to(torch.int32).repeat_interleave(2)[::2]
    assert strided[buffer].numel() > 1 and not strided[buffer].is_contiguous()
    with pytest.raises(ValueError, match="tensors must be contiguous"):
        call(**strided)
    torch.cuda.synchronize()
    for name in outputs:    # nothing was launched
        assert args[name].tolist() == [FILL], name


def test_the_same_calls_well_typed_give_what_they_gave():
    import torch
    _, call, args, _, _ = _inflate()
    out_len, status, _ = call(**args)
    assert (out_len.tolist(), status.tolist()) == ([0], [0])
    _, call, args, _, _ = _expand()
    assert call(**args).tolist() == [0] and args["rgba"].tolist() == [0x42, 0x42, 0x42, 255]
    _, call, args, _, _ = _crc()
    crc, status = call(**args)
    assert (crc.item() & 0xFFFFFFFF, status.tolist()) == (0x352441C2, [0])
    torch.cuda.synchronize()
