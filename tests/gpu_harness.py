"""Helpers for the -m gpu parity tests: pack streams, run the HIP path through the C ABI
(fdeflate_amd.inflate_batch / deflate_ultrafast_batch) and the oracle on the same bytes."""
import zlib

import numpy as np

import oracle_binding as ob
import streams


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


def gpu_inflate(blobs, caps, flags=0, guard=5, fill=0xA5):
    """Decodes blobs[i] into a slot of caps[i] bytes.  Slots are interleaved with `guard`-byte
    dummy slots (empty input) so every slot starts at an odd alignment and any out-of-slot write
    is detected.  -> (status, out_len, adler, outputs[list of bytes], guards_ok)"""
    import torch
    import fdeflate_amd as fd

    n = len(blobs)
    all_blobs, all_caps = [], []
    for b, c in zip(blobs, caps):
        all_blobs += [b, b""]
        all_caps += [c, guard]
    buf, in_off = streams.pack_exact(all_blobs)
    out_off = np.zeros(2 * n + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum(np.asarray(all_caps, dtype=np.uint64))
    total = int(out_off[-1])
    d_in = _t(buf)
    d_in_off = _t(in_off.astype(np.int64))
    d_out = torch.full((max(total, 1),), fill, dtype=torch.uint8, device="cuda")
    d_out_off = _t(out_off.astype(np.int64))
    out_len, status, adler = fd.inflate_batch(d_in, d_in_off, d_out, d_out_off, flags=flags)
    torch.cuda.synchronize()
    h_out = d_out.cpu().numpy()
    st = status.cpu().numpy().view(np.uint32)[0::2]
    ln = out_len.cpu().numpy().view(np.uint32)[0::2]
    ad = adler.cpu().numpy().view(np.uint32)[0::2]
    outs, guards_ok = [], True
    for i in range(n):
        o0, o1, g1 = int(out_off[2 * i]), int(out_off[2 * i + 1]), int(out_off[2 * i + 2])
        outs.append(h_out[o0:o1])
        if not np.all(h_out[o1:g1] == fill):
            guards_ok = False
    return st, ln, ad, outs, guards_ok


_CHUNK = 1 << 28   # device comparisons of big slots go 256 MiB at a time (the temporaries stay small)


def _all_fill(t, fill):
    """Device reduction: every byte of the uint8 tensor `t` is `fill`."""
    for c in range(0, t.numel(), _CHUNK):
        if not bool((t[c:c + _CHUNK] == fill).all()):
            return False
    return True


def _equal_on_device(t, expected):
    """torch.equal of the device tensor `t` with host bytes `expected` (same length), uploaded in pieces."""
    import torch
    e = np.frombuffer(expected, dtype=np.uint8)
    assert e.size == t.numel()
    for c in range(0, e.size, _CHUNK):
        if not torch.equal(t[c:c + _CHUNK], torch.from_numpy(e[c:c + _CHUNK].copy()).cuda()):
            return False
    return True


def pad_to(blob, n, seed=1):
    """`blob` brought to exactly n bytes by junk behind its Adler-32 trailer (which a decoder ignores)."""
    assert len(blob) <= n, (len(blob), n)
    junk = np.random.default_rng(seed).integers(1, 256, n - len(blob), dtype=np.uint8).tobytes()
    return bytes(blob) + junk


class DeviceSlots:
    """The output slots of one gpu_inflate_big call, still on the device."""

    def __init__(self, d_out, out_off, fill):
        self.d_out, self.out_off, self.fill = d_out, out_off, fill

    def head_equals(self, i, data):
        """The first len(data) bytes of slot i are `data` (bytes / uint8 array; uploaded, torch.equal)."""
        o0, o1 = int(self.out_off[2 * i]), int(self.out_off[2 * i + 1])
        assert len(data) <= o1 - o0
        return _equal_on_device(self.d_out[o0:o0 + len(data)], data)

    def untouched(self, i, start=0):
        """Slot i still holds the fill byte from byte `start` to its end (device reduction)."""
        o0, o1 = int(self.out_off[2 * i]), int(self.out_off[2 * i + 1])
        return _all_fill(self.d_out[min(o0 + start, o1):o1], self.fill)


def gpu_inflate_big(blobs, caps, flags=0, guard=5, fill=0xA5):
    """gpu_inflate for slots too large to bring back: the same odd guard slots, but every comparison stays on the
    device -- expected bytes are uploaded per stream and compared with torch.equal (DeviceSlots.head_equals), untouched
    parts of a slot and the guard slots are checked against `fill` by a device reduction.  Only status / length /
    Adler-32 come to the host.  -> (status, out_len, adler, slots[DeviceSlots], guards_ok)"""
    import torch
    import fdeflate_amd as fd

    n = len(blobs)
    in_off = np.zeros(2 * n + 1, dtype=np.int64)
    in_off[1::2] = [len(b) for b in blobs]
    in_off = np.cumsum(in_off)
    d_in = torch.zeros(max(int(in_off[-1]), 1), dtype=torch.uint8, device="cuda")
    for i, b in enumerate(blobs):
        a = np.frombuffer(b, dtype=np.uint8)
        for c in range(0, a.size, _CHUNK):
            o = int(in_off[2 * i]) + c
            piece = a[c:c + _CHUNK]
            d_in[o:o + piece.size] = torch.from_numpy(piece.copy()).cuda()
    out_off = np.zeros(2 * n + 1, dtype=np.int64)
    out_off[1::2] = caps
    out_off[2::2] = guard
    out_off = np.cumsum(out_off)
    d_out = torch.full((max(int(out_off[-1]), 1),), fill, dtype=torch.uint8, device="cuda")
    out_len, status, adler = fd.inflate_batch(d_in, torch.from_numpy(in_off).cuda(), d_out, torch.from_numpy(out_off).cuda(),
                                              flags=flags)
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint32)[0::2]
    ln = out_len.cpu().numpy().view(np.uint32)[0::2]
    ad = adler.cpu().numpy().view(np.uint32)[0::2]
    guards_ok = all(_all_fill(d_out[int(out_off[2 * i + 1]):int(out_off[2 * i + 2])], fill) for i in range(n))
    return st, ln, ad, DeviceSlots(d_out, out_off, fill), guards_ok


def encoder_guard_faults(h, out_off, ln, empty, fill):
    """The guard slots (odd entries) of an encoder batch: each holds the stream of an empty input, `empty`, and behind it
    bytes that nobody may write -- still `fill`.  -> list of faults (empty: all is well)"""
    faults = []
    for i in range(1, len(out_off) - 1, 2):
        g = h[int(out_off[i]):int(out_off[i + 1])]
        if int(ln[i]) != len(empty) or g[:len(empty)].tobytes() != empty:
            faults.append((i // 2, "guard slot's empty stream damaged", int(ln[i]), g[:len(empty)].tobytes().hex()))
        if not np.all(g[len(empty):] == fill):
            faults.append((i // 2, "guard bytes changed", g[len(empty):].tobytes().hex()))
    return faults


def gpu_encode_slots(encode, raws, caps, empty, guard=3, fill=0x5A):
    """Runs a batched encoder into slots of caps[i] bytes, packed back to back at odd alignments.  Behind each comes a
    guard slot: an empty input, whose stream `empty` fits, and `guard` bytes more that must keep the fill byte.
    encode(d_in, d_in_off, d_out, d_out_off) -> out_len tensor.
    -> (out_len[n] uint32, slots[list of uint8 arrays: the whole slot], guard_faults[empty list: all is well])"""
    import torch

    n = len(raws)
    all_raw, all_caps = [], []
    for r, c in zip(raws, caps):
        all_raw += [r, b""]
        all_caps += [c, len(empty) + guard]
    buf, in_off = streams.pack_exact(all_raw)
    out_off = np.zeros(2 * n + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(np.asarray(all_caps, dtype=np.int64))
    d_out = torch.full((max(int(out_off[-1]), 1),), fill, dtype=torch.uint8, device="cuda")
    out_len = encode(_t(buf), _t(in_off.astype(np.int64)), d_out, _t(out_off))
    torch.cuda.synchronize()
    h = d_out.cpu().numpy()
    ln = out_len.cpu().numpy().view(np.uint32)
    slots = [h[int(out_off[2 * i]):int(out_off[2 * i + 1])] for i in range(n)]
    return ln[0::2], slots, encoder_guard_faults(h, out_off, ln, empty, fill)


def oracle_inflate(blobs, caps, ignore_adler32=False):
    sts, lens, ads, outs = [], [], [], []
    for b, c in zip(blobs, caps):
        st, out, ad = ob.decompress_bounded(b, c, ignore_adler32)
        sts.append(st)
        lens.append(len(out))
        ads.append(ad)
        outs.append(out)
    return sts, lens, ads, outs


def assert_inflate_parity(names, blobs, caps, flags=0):
    """Bit-exact: status for every stream; length, bytes and Adler-32 whenever the reference
    defines them (Ok and OutputTooLarge)."""
    st, ln, ad, outs, guards_ok = gpu_inflate(blobs, caps, flags)
    rs, rl, ra, ro = oracle_inflate(blobs, caps, bool(flags & 1))
    bad = []
    for i, name in enumerate(names):
        if int(st[i]) != rs[i]:
            bad.append((name, "status", ob.STATUS_NAMES[int(st[i])] if st[i] < 18 else int(st[i]),
                        ob.STATUS_NAMES[rs[i]], caps[i]))
            continue
        if rs[i] in (0, 17):
            if int(ln[i]) != rl[i]:
                bad.append((name, "len", int(ln[i]), rl[i], caps[i]))
            elif outs[i][:rl[i]].tobytes() != ro[i]:
                diff = np.nonzero(np.frombuffer(ro[i], dtype=np.uint8) != outs[i][:rl[i]])[0]
                bad.append((name, "bytes", "first diff at %d of %d" % (diff[0], rl[i]), caps[i]))
            elif rs[i] == 0 and int(ad[i]) != ra[i]:
                bad.append((name, "adler", hex(int(ad[i])), hex(ra[i])))
    assert guards_ok, "a kernel wrote outside its output slot"
    assert not bad, bad[:10]


def gpu_deflate(raws, guard=3, slack=0, fill=0x5A):
    import torch
    import fdeflate_amd as fd

    n = len(raws)
    all_raw, all_caps = [], []
    for r in raws:
        all_raw += [r, b""]
        all_caps += [fd.ultrafast_bound(len(r)) + slack, fd.ultrafast_bound(0) + guard]
    buf, in_off = streams.pack_exact(all_raw)
    out_off = np.zeros(2 * n + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum(np.asarray(all_caps, dtype=np.uint64))
    d_in = _t(buf)
    d_out = torch.full((int(out_off[-1]),), fill, dtype=torch.uint8, device="cuda")
    out_len = fd.deflate_ultrafast_batch(d_in, _t(in_off.astype(np.int64)), d_out, _t(out_off.astype(np.int64)))
    torch.cuda.synchronize()
    h = d_out.cpu().numpy()
    ln = out_len.cpu().numpy().view(np.uint32)
    res = []
    ok = True
    for i in range(n):
        o0 = int(out_off[2 * i])
        res.append(h[o0:o0 + int(ln[2 * i])].tobytes())
        o1 = int(out_off[2 * i + 1])
        if not np.all(h[o0 + int(ln[2 * i]):o1] == fill):
            ok = False  # wrote past its own length inside the slot
    return res, ok


# ---- fdh_inflate_batch_resumable ----

def drive_resumable(fd, comps, in_cuts, out_cuts, per_call=False):
    """All streams side by side in one batch; call k sees input up to in_cuts[i][k] and room up to out_cuts[i][k].
    A slot is [out_off[j], out_off[j + 1]): the room a stream does not have yet is the slot of an empty stream
    behind it (2n streams per call, every other one of length zero: InsufficientInput, nothing written).  The
    input is packed anew for every call -- only the output has to stay where it is."""
    import torch
    n = len(comps)
    cap = [oc[-1] for oc in out_cuts]
    out_base = np.zeros(n + 1, dtype=np.int64)
    out_base[1:] = np.cumsum([c + 16 for c in cap])
    d_out = torch.full((int(out_base[-1]),), 0xA5, dtype=torch.uint8, device="cuda")
    resume = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    steps = max(max(len(x) for x in in_cuts), max(len(x) for x in out_cuts))
    res = None
    for k in range(steps):
        io = np.zeros(2 * n + 1, dtype=np.int64)
        oo = np.zeros(2 * n + 1, dtype=np.int64)
        parts = []
        pos = 0
        for i in range(n):
            cut = in_cuts[i][min(k, len(in_cuts[i]) - 1)]
            parts.append(comps[i][:cut])
            io[2 * i] = pos
            pos += cut
            io[2 * i + 1] = pos
            oo[2 * i] = out_base[i]
            oo[2 * i + 1] = out_base[i] + out_cuts[i][min(k, len(out_cuts[i]) - 1)]
        io[2 * n] = pos
        oo[2 * n] = out_base[n]
        d_in = torch.from_numpy(np.frombuffer(b"".join(parts) + bytes(16), dtype=np.uint8).copy()).cuda()
        r2 = torch.zeros((2 * n, 4), dtype=torch.int32, device="cuda")
        r2[0::2] = resume
        ln, st, ad = fd.inflate_batch_resumable(d_in, torch.from_numpy(io).cuda(), d_out, torch.from_numpy(oo).cuda(), r2,
                                                resume_in=(k > 0))
        torch.cuda.synchronize()
        resume = r2[0::2].contiguous()
        res = (ln.cpu().numpy().view(np.uint32)[0::2].copy(), st.cpu().numpy().view(np.uint32)[0::2].copy(),
               ad.cpu().numpy().view(np.uint32)[0::2].copy())
        if per_call:
            # every call on its own: status, length and bytes so far are those of the reference's streaming `read`
            # given the same input prefix and the same room in one go (src/decompress.rs:158-219 through the
            # one-shot classification of :1111-1144), and a record is left exactly where the stream can go on
            hk = d_out.cpu().numpy()
            rk = resume.cpu().numpy()
            for i in range(n):
                cut = in_cuts[i][min(k, len(in_cuts[i]) - 1)]
                room = out_cuts[i][min(k, len(out_cuts[i]) - 1)]
                est, eout, _ = ob.decompress_bounded(comps[i][:cut], room)
                assert int(res[1][i]) == est, (k, i, int(res[1][i]), est)
                if est in (0, 17):
                    assert int(res[0][i]) == len(eout) and hk[out_base[i]:out_base[i] + len(eout)].tobytes() == eout, (k, i)
                if est == 2:
                    d = ob.Decompressor()
                    buf = np.zeros(max(room, 1), dtype=np.uint8)
                    _, _, produced = d.read(comps[i][:cut], buf[:room], 0)
                    assert int(res[0][i]) == produced, (k, i, int(res[0][i]), produced)
                    assert hk[out_base[i]:out_base[i] + produced].tobytes() == buf[:produced].tobytes(), (k, i)
                if est not in (2, 17):
                    assert not rk[i].any(), (k, i, est, rk[i])  # "all zero for every other status"
                else:
                    # the record names a place inside what the call delivered, and its Adler word is the Adler-32 of
                    # the bytes in front of that place (the call that goes on there starts its sums from it)
                    rec = rk[i].view(np.uint32)
                    opos = int(rec[2])
                    if rec[0] == 0:
                        # "no resume point" (include/fdeflate_hip.h: header_bit 0, the record all zero: go on from the
                        # first byte).  Only for a call that delivered nothing: these streams lie far below the one gate
                        # of the records (bit position < 2^30, DESIGN.md "Size gates"), so in front of any delivered
                        # byte there is the start of a decoding step to name -- a record cleared by mistake would
                        # otherwise cost only time and go unnoticed
                        assert not rec.any() and int(res[0][i]) == 0, (k, i, est, rec.tolist(), int(res[0][i]))
                    else:
                        assert opos <= int(res[0][i]), (k, i, est, rec.tolist(), int(res[0][i]))
                        assert int(rec[3]) == zlib.adler32(hk[out_base[i]:out_base[i] + opos].tobytes()), (k, i, est, rec.tolist())
    h = d_out.cpu().numpy()
    outs = [h[out_base[i]:out_base[i] + cap[i]] for i in range(n)]
    guards = all((h[out_base[i] + cap[i]:out_base[i + 1]] == 0xA5).all() for i in range(n))
    return res, outs, guards, resume.cpu().numpy()
