"""The Adler-32 worst-case payloads and their streams, on the CPU: the byte-at-a-time model against zlib.adler32 and
the oracle, and every stream of tests/adler_payloads.py through the oracle's decoder."""
import zlib

import numpy as np
import pytest

import adler_payloads as ap
import oracle_binding as ob


def test_model_known_values():
    assert ap.adler32_model(b"") == 1
    assert ap.adler32_model(b"Wikipedia") == 0x11E60398
    assert ap.adler32_model(b"pedia", ap.adler32_model(b"Wiki")) == 0x11E60398


def test_maximal_state_after_46764_bytes_of_ff():
    """A = B = 65 520, the largest value the two halves can have together, after 46 764 bytes of 0xFF and again
    every 65 521 bytes -- and at no shorter length."""
    a, b, hits = 1, 0, []
    for n in range(1, 46764 + ap.MOD + 1):
        a = (a + 255) % ap.MOD
        b = (b + a) % ap.MOD
        if a == b == ap.MOD - 1:
            hits.append(n)
    assert tuple(hits) == ap.MAXIMAL_STATE_LENGTHS == (46764, 112285)
    assert ap.adler32_model(ap.ff(46764)) == 0xFFF0FFF0 == zlib.adler32(ap.ff(46764))
    assert zlib.adler32(ap.ff(112285)) == 0xFFF0FFF0


@pytest.mark.parametrize("kind", list(ap.PAYLOADS))
def test_payloads_are_what_they_claim(kind):
    for n in ap.LENGTHS:
        raw = ap.payload(kind, n)
        assert len(raw) == n and raw == ap.PAYLOADS[kind](n)      # the length, and the same bytes every time
    x = np.frombuffer(ap.payload(kind, (1 << 20) + 3), dtype=np.uint8)
    n = x.size
    heavy = x >= 0xF8
    assert np.all(heavy | (x == 0))
    if kind == "ff":
        assert np.all(x == 0xFF)
    elif kind == "high":
        assert heavy.all() and abs(float(x.mean()) - 251.5) < 0.05
        assert int(np.max(np.diff(np.nonzero(np.diff(x))[0]))) < 16     # no long run of one literal
    elif kind == "ff_sparse":
        assert 0.45 < float(heavy.mean()) < 0.55
        edges = np.nonzero(np.diff(heavy.astype(np.int8)))[0]
        assert 1 <= int(np.diff(edges).min()) and int(np.diff(edges).max()) <= 600
    elif kind == "ff_front":
        assert heavy[:(n + 3) // 4].all() and not heavy[(n + 3) // 4:].any()
    else:
        assert heavy[n - (n + 3) // 4:].all() and not heavy[:n - (n + 3) // 4].any()


@pytest.mark.parametrize("kind", list(ap.PAYLOADS))
def test_model_zlib_and_oracle_agree_on_every_payload(kind):
    for n in ap.LENGTHS:
        raw = ap.payload(kind, n)
        want = ap.adler32_model(raw)
        assert zlib.adler32(raw) == want, (kind, n)
        assert ob.adler32(raw) == want, (kind, n)


@pytest.mark.parametrize("kind", list(ap.PAYLOADS))
def test_every_stream_decodes_in_the_oracle_with_the_model_sum(kind):
    for n in ap.LENGTHS:
        raw = ap.payload(kind, n)
        want = ap.adler32_model(raw) if n <= 250000 else zlib.adler32(raw)     # (equal: the test above)
        for enc in ap.ENCODINGS:
            comp = ap.stream(kind, n, enc)
            assert int.from_bytes(comp[-4:], "big") == want, (kind, n, enc)
            st, out, ad = ob.decompress_bounded(comp, n)
            assert st == 0 and ad == want and out == raw, (kind, n, enc, st, hex(ad), hex(want))
            assert zlib.decompress(comp) == raw, (kind, n, enc)


def test_sizes_of_the_ff_streams():
    """Three bits per 0xFF byte in the ultra-fast format, about one per byte Huffman-only, a handful of long matches
    at level 1 / RLE: the three shapes of stream the decoders see."""
    n = 1 << 20
    assert len(ap.stream("ff", n, "uf")) == 393276
    assert len(ap.stream("ff", n, "level1")) == len(ap.stream("ff", n, "rle")) == 1070
    assert n // 8 < len(ap.stream("ff", n, "huff")) < n // 8 + 1024
