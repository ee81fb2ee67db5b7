"""Token-level writer of deflate streams: tokens in, (stream bytes, payload bytes) out.

Every valid stream of the other suites comes from zlib or from this project's encoders; this helper writes the valid
streams that neither of them writes -- run tokens behind a non-zero byte, runs cut off the ultra-fast encoder's
grammar, every (length, distance) at every ring phase, codes of every table class of the LZ-window kernel, headers
with every HLIT / HDIST / HCLEN and repeat count, blocks of every kind in every order.  The payload of a stream is
produced by the writer itself while it writes (a match is `out.append(out[-dist])`, byte by byte), so a test has
three independent answers: the writer's payload, zlib.decompress and the oracle.

Deterministic from its seeds.  Uses numpy and zlib only; the ultra-fast code and prefix come from
tests/golden/constants.json (tests/test_deflate_gen.py checks the prefix against the oracle's encoder).
Not a test module.
"""
import hashlib
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
            131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
             2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLCL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
EOB = 256

_LEN_SYM = [0] * 259          # length -> index of its length symbol (258 -> 28)
for _i, _b in enumerate(LEN_BASE):
    for _l in range(_b, min(_b + (1 << LEN_EXTRA[_i]), 259)):
        _LEN_SYM[_l] = _i
_LEN_SYM[258] = 28


def dist_symbol(dist):
    lo, hi = 0, 29
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if DIST_BASE[mid] <= dist:
            lo = mid
        else:
            hi = mid - 1
    return lo


# --------------------------------------------------------------------------------------
# bits
# --------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bit writer that flushes whole bytes to a bytearray (linear in the stream length)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k
        return self

    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.bits(0, -self.n & 7)
        k = self.n >> 3
        self.buf += self.acc.to_bytes(k, "little")
        self.acc, self.n = 0, 0
        return self

    def raw(self, data):
        self.align()
        self.buf += data
        return self

    def many(self, codes, lens):
        """codes[i] in lens[i] bits each, in order (numpy arrays; a code has up to 15 bits): the vectorised `bits`."""
        lens = np.asarray(lens, dtype=np.int64)
        if lens.size == 0:
            return self
        codes = np.asarray(codes, dtype=np.int64)
        head = self.n
        pos = head + np.cumsum(lens) - lens
        total = int(pos[-1] + lens[-1])
        arr = np.zeros((total + 7) & ~7, dtype=np.uint8)
        for k in range(head):
            arr[k] = (self.acc >> k) & 1
        for k in range(int(lens.max())):
            m = lens > k
            arr[pos[m] + k] = (codes[m] >> k) & 1
        packed = np.packbits(arr, bitorder="little")
        whole = total >> 3
        self.buf += packed[:whole].tobytes()
        self.n = total & 7
        self.acc = int(packed[whole]) & ((1 << self.n) - 1) if self.n else 0
        return self

    def tobytes(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> per symbol (bit-reversed code, length) or None"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [None] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            out[s] = (int(format(nxt[l], "0%db" % l)[::-1], 2), l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """sum of 2^-l over the used symbols, in units of 2^-15 (32768: complete)"""
    return sum(1 << (15 - l) for l in lengths if l)


# --------------------------------------------------------------------------------------
# code builders
# --------------------------------------------------------------------------------------
def complete_code(n, max_len, r, deep=0.5, at_max=0):
    """Lengths of a complete prefix code of n >= 2 leaves, none longer than max_len, by Kraft filling: a leaf is split
    in two until there are n.  `deep` is the chance that the deepest leaf that can still be split is taken instead of
    a random one (0: bushy, codes of about log2(n) bits; 1: one long chain).  at_max: at least that many leaves of
    exactly max_len bits.  -> list of n lengths, ascending."""
    assert 2 <= n <= (1 << max_len)
    leaves = [1, 1]
    while len(leaves) < n:
        room = n - len(leaves)
        cand = [i for i, l in enumerate(leaves) if l < max_len]
        # keep it feasible: the shallow leaves that are left must be able to take the rest
        pick = None
        short = at_max - sum(1 for l in leaves if l == max_len)
        if short > 0 and room <= (short + 1) // 2 + 1:
            deepest = max(leaves[i] for i in cand)
            pick = [i for i in cand if leaves[i] == deepest][0]
        elif r.random() < deep:
            deepest = max(leaves[i] for i in cand)
            pick = [i for i in cand if leaves[i] == deepest][0]
        else:
            pick = cand[int(r.integers(0, len(cand)))]
        l = leaves.pop(pick)
        leaves += [l + 1, l + 1]
    assert kraft(leaves) == 32768
    return sorted(leaves)


def shaped_code(n, index_bits, long_lengths, r, deep=0.3):
    """A complete code of n leaves whose codes beyond index_bits bits are exactly `long_lengths` (their Kraft sum a
    whole number q of 2^-index_bits: in canonical order they fill the last q primary prefixes of a table with
    `index_bits` index bits, the shorter ones first); every other code fits the index."""
    w = sum(1 << (15 - l) for l in long_lengths)
    q, rest = divmod(w, 1 << (15 - index_bits))
    assert rest == 0 and all(l > index_bits for l in long_lengths)
    base = complete_code(n - len(long_lengths) + q, index_bits, r, deep, at_max=q)
    assert sum(1 for l in base if l == index_bits) >= q, (base, q)
    out = sorted(base)[:len(base) - q] + sorted(long_lengths)
    assert len(out) == n and kraft(out) == 32768
    return out


def chain(index_bits, d):
    """index_bits + 1, + 2, .., d, d: the long codes of one primary prefix, the longest of d bits"""
    return list(range(index_bits + 1, d + 1)) + [d]


def spread(lengths, symbols, r, size):
    """The lengths handed to `symbols` in a seeded random order -> list of `size` code lengths (0: no code)."""
    assert len(lengths) == len(symbols)
    out = [0] * size
    order = r.permutation(len(symbols))
    for k, l in zip(order, lengths):
        out[symbols[int(k)]] = int(l)
    return out


def classify_code(lengths, index_bits, cap):
    """Which decode paths of a two-level table a code needs (inflate_lz.h, lz_build_sub_t): the codes longer than
    index_bits share primary prefixes (their low index_bits stream bits); a prefix whose longest code has m bits asks
    for 2^(m - index_bits) second-level entries, handed out in ascending prefix order from `cap` entries; the offset
    runs on over a prefix that did not fit.  -> (class, histogram) with class one of
        none          no code beyond the index
        second_level  every long prefix got its entries
        overflow      some did, some take the canonical walk
        walk_only     none did
    and histogram = dict(prefixes=.., entries=.., fitted=..)."""
    longest = {}
    for c in canonical_codes(lengths):
        if c is not None and c[1] > index_bits:
            p = c[0] & ((1 << index_bits) - 1)
            longest[p] = max(longest.get(p, 0), c[1])
    off = fitted = 0
    for p in sorted(longest):
        sz = 1 << (longest[p] - index_bits)
        if off + sz <= cap:
            fitted += 1
        off += sz
    hist = dict(prefixes=len(longest), entries=off, fitted=fitted)
    if not longest:
        return "none", hist
    if fitted == len(longest):
        return "second_level", hist
    return ("overflow" if fitted else "walk_only"), hist


TABLE_CLASSES = ("none", "second_level", "overflow", "walk_only")


def code_of_class(cls, n, index_bits, cap, r):
    """Lengths of a complete code of n symbols that classify_code(.., index_bits, cap) calls `cls`, or None where no
    such code exists (one prefix never asks for more than 2^(15 - index_bits) entries, so with cap at or above that
    the first prefix always fits and nothing is walk_only).  The candidates: one chain to the deepest length that
    still fits `cap`; whole blocks of codes of that length over several prefixes; a short pair in front of them."""
    if cls == "none":
        return complete_code(n, index_bits, r, deep=0.1)
    d = index_bits + 1
    while d < 15 and (2 << (d - index_bits)) <= cap:
        d += 1                                        # the deepest code whose prefix fits `cap` on its own
    per = 1 << (d - index_bits)
    cands = []
    if cls == "second_level":
        cands = [[d] * (2 * per), chain(index_bits, d)]
    elif cls == "overflow":
        cands = [[index_bits + 1] * 2 + [d] * (per * (cap // per)), chain(index_bits, d) * 2, chain(index_bits, 15) + chain(index_bits, d)]
    elif cls == "walk_only":
        cands = [chain(index_bits, 15)]
    for long_lengths in cands:
        if len(long_lengths) > n - 8 or (1 << (d - index_bits)) > cap and cls != "walk_only":
            continue
        lens = shaped_code(n, index_bits, long_lengths, r)
        if classify_code(lens, index_bits, cap)[0] == cls:
            return lens
    return None


# --------------------------------------------------------------------------------------
# the stream writer
# --------------------------------------------------------------------------------------
def M(length, dist, long258=False, dsym=None, dbits=None):
    """A match token.  long258: length 258 written as symbol 284 with extra bits 31; dsym: that distance symbol
    whatever the distance (error streams); dbits: (value, nbits) raw bits in place of the distance code."""
    return (length, dist, long258, dsym, dbits)


def rle_lengths(seq, use16=True, use17=True, use18=True):
    """The greedy run-length form of a sequence of code lengths -> list of (code-length symbol, extra value)."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11 and use18:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            while run >= 3 and use17:
                k = min(run, 10)
                out.append((17, k - 3))
                run -= k
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3 and use16:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


def expand_cl_syms(cl_syms):
    out = []
    for s, e in cl_syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        elif s == 17:
            out += [0] * (3 + e)
        else:
            out += [0] * (11 + e)
    return out


def cl_code_for(cl_syms, r, hclen=None):
    """A complete code-length code (lengths up to 7) over the symbols `cl_syms` uses -- with one more symbol when they
    use only one; the more often a symbol is used, the shorter its code."""
    used = {}
    for s, _ in cl_syms:
        used[s] = used.get(s, 0) + 1
    if len(used) == 1:
        allowed = CLCL_ORDER[:hclen] if hclen else CLCL_ORDER
        used[[s for s in allowed if s not in used][0]] = 0
    syms = sorted(used, key=lambda s: -used[s])
    lens = complete_code(len(syms), 7, r, deep=0.4)
    cl = [0] * 19
    for s, l in zip(syms, lens):
        cl[s] = l
    return cl


class StreamWriter:
    """One zlib stream, block by block.  `out` is the payload so far."""

    def __init__(self, header=b"\x78\x01"):
        self.w = BitWriter()
        self.w.raw(header)
        self.out = bytearray()
        self.stored_phases = []       # (bit phase of the block header, payload length) of every stored block
        self.matches = []             # (length, dist) in stream order
        self.block_bits = []          # (first bit, end bit) of every Huffman block's data
        self.cl_syms = []             # every (code-length symbol, extra) written
        self.lenient = False          # error streams: a match may reach in front of the payload (it reads zeros)

    # ---- blocks ----
    def stored(self, data, final=False):
        assert len(data) <= 65535
        self.stored_phases.append((self.w.bitpos() & 7, len(data)))
        self.w.bits(1 if final else 0, 1).bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16).bits(len(data) ^ 0xFFFF, 16)
        self.w.raw(bytes(data))
        self.out += data
        return self

    def fixed(self, tokens, final=False):
        self.w.bits(1 if final else 0, 1).bits(1, 2)
        return self._tokens(tokens, canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST))

    def dynamic(self, tokens, lit_lengths, dist_lengths, final=False, hlit=None, hdist=None, hclen=None,
                cl_lengths=None, cl_syms=None, r=None):
        """hlit / hdist / hclen default to the least the codes need; cl_syms defaults to the greedy run-length form of
        the lengths, cl_lengths to a complete code over the symbols cl_syms uses."""
        r = r if r is not None else np.random.default_rng(1)
        need_l = max([257] + [s + 1 for s, l in enumerate(lit_lengths) if l])
        need_d = max([1] + [s + 1 for s, l in enumerate(dist_lengths) if l])
        hlit = need_l if hlit is None else hlit
        hdist = need_d if hdist is None else hdist
        assert need_l <= hlit <= 286 and need_d <= hdist <= 30
        seq = (list(lit_lengths) + [0] * 286)[:hlit] + (list(dist_lengths) + [0] * 30)[:hdist]
        if cl_syms is None:
            cl_syms = rle_lengths(seq)
        assert expand_cl_syms(cl_syms) == seq, "the code-length symbols do not spell the lengths"
        if cl_lengths is None:
            cl_lengths = cl_code_for(cl_syms, r, hclen)
        need_c = max([4] + [i + 1 for i in range(19) if cl_lengths[CLCL_ORDER[i]]])
        hclen = need_c if hclen is None else hclen
        assert need_c <= hclen <= 19 and kraft(cl_lengths) == 32768 and max(cl_lengths) <= 7
        w = self.w
        w.bits(1 if final else 0, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lengths[CLCL_ORDER[i]], 3)
        cc = canonical_codes(cl_lengths)
        for s, e in cl_syms:
            w.bits(*cc[s])
            if s >= 16:
                w.bits(e, (2, 3, 7)[s - 16])
        self.cl_syms += cl_syms
        return self._tokens(tokens, canonical_codes((list(lit_lengths) + [0] * 286)[:286]),
                            canonical_codes((list(dist_lengths) + [0] * 30)[:30]))

    # ---- tokens ----
    def _tokens(self, tokens, lc, dc):
        """A token is an int (literal, or EOB = 256), a bytes-like (that many literals) or M(..).  The block ends at
        EOB; one is added when the tokens do not end with it."""
        w, out = self.w, self.out
        first = w.bitpos()
        lit_code = np.array([c[0] if c else 0 for c in lc[:256]], dtype=np.int64)
        lit_len = np.array([c[1] if c else 0 for c in lc[:256]], dtype=np.int64)
        ended = False
        for t in tokens:
            assert not ended, "a token behind the end-of-block"
            if isinstance(t, (bytes, bytearray)) and len(t) <= 16:
                for b in t:
                    w.bits(*lc[b])
                out += t
            elif isinstance(t, (bytes, bytearray, np.ndarray)):
                a = np.frombuffer(bytes(t), dtype=np.uint8)
                assert lit_len[a].all(), "a literal without a code"
                w.many(lit_code[a], lit_len[a])
                out += a.tobytes()
            elif isinstance(t, tuple):
                length, dist, long258, dsym, dbits = t
                ls = 27 if (long258 and length == 258) else _LEN_SYM[length]
                w.bits(*lc[257 + ls]).bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
                if dbits is not None:
                    w.bits(*dbits)
                else:
                    ds = dist_symbol(dist) if dsym is None else dsym
                    w.bits(*dc[ds])
                    if ds < 30:
                        w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
                self.matches.append((length, dist))
                if dist > len(out):
                    assert self.lenient, "a match reaches in front of the payload"
                    out[:0] = bytes(dist - len(out))
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
            elif t == EOB:
                w.bits(*lc[256])
                ended = True
            else:
                w.bits(*lc[t])
                out.append(t)
        if not ended:
            w.bits(*lc[256])
        self.block_bits.append((first, w.bitpos()))
        return self

    def finish(self, adler=None):
        a = zlib.adler32(bytes(self.out)) if adler is None else adler
        self.w.raw(a.to_bytes(4, "big"))
        return self.w.tobytes(), bytes(self.out)

    def done(self):
        """finish() and what the coverage assertions of tests/test_deflate_gen.py count -> (stream, payload, info)"""
        comp, raw = self.finish()
        return comp, raw, dict(matches=self.matches, block_bits=self.block_bits, cl_syms=self.cl_syms,
                               stored_phases=self.stored_phases)


# --------------------------------------------------------------------------------------
# behind the ultra-fast prefix
# --------------------------------------------------------------------------------------
_constants = None


def constants():
    global _constants
    if _constants is None:
        with open(os.path.join(GOLDEN, "constants.json")) as f:
            _constants = json.load(f)
    return _constants


def uf_prefix():
    """-> (the 53 whole bytes, the low 5 bits of byte 53) in front of an ultra-fast stream's first token"""
    h = constants()["ULTRAFAST_HEADER"]
    return bytes(h[:53]), h[53] & 31


def uf_foreign(tokens, end=True, adler=None, lenient=False):
    """The ultra-fast encoder's prefix (zlib header, block header and code: 53 bytes + 5 bits), then `tokens` in the
    ultra-fast code -- HUFFMAN_LENGTHS, one distance code of one bit, value 0: every match has distance 1 -- then
    end-of-block and the Adler-32.  -> (stream, payload)"""
    sw = StreamWriter(header=b"")
    sw.lenient = lenient
    head, low = uf_prefix()
    sw.w.raw(head)
    sw.w.bits(low, 5)
    sw._tokens(list(tokens) + ([EOB] if end else []), canonical_codes(constants()["HUFFMAN_LENGTHS"]), [(0, 1)] + [None] * 29)
    return sw.finish(adler) if end else (sw.w.tobytes(), bytes(sw.out))


UF_POLICIES = ("reference", "any_byte", "threes", "fours", "tail_first", "random_cuts", "literals_only")


def _stretches(a, zero_only):
    """maximal stretches of equal bytes -> (starts, ends)"""
    if a.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cut = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [a.size]))
    if zero_only:
        keep = a[starts] == 0
        starts, ends = starts[keep], ends[keep]
    return starts, ends


def _cut_run(n, policy, r):
    """How a policy writes the n bytes of a run behind its first literal -> list of match lengths and, last, the
    number of literals that finish it.  (reference / any_byte: 258s, then one token of 5..257 or up to four
    literals -- src/compress/ultrafast.rs:45-66.)"""
    if policy in ("reference", "any_byte", "tail_first"):
        k, rem = divmod(n, 258)
        tail, lits = ([rem], 0) if rem > 4 else ([], rem)
        return ([258] * k + tail, lits) if policy != "tail_first" else (tail + [258] * k, lits)
    if policy in ("threes", "fours"):
        q = 3 if policy == "threes" else 4
        return [q] * (n // q), n % q
    assert policy == "random_cuts"
    cuts = []
    while n >= 3:
        s = int(r.integers(0, 29))
        length = min(LEN_BASE[s] + int(r.integers(0, 1 << LEN_EXTRA[s])), 258, n)
        cuts.append(length)
        n -= length
    return cuts, n


def uf_parse(raw, policy, seed=0, long258=False):
    """A buffer as tokens for uf_foreign, under a named policy (one payload, many streams):
        reference      the encoder's grammar: runs of zeros only, and only those the encoder finds -- it looks at
                       8-byte words, so a stretch of zeros is a run when it holds the last byte of a word of the
                       part of the buffer that is whole words; a zero, 258-byte tokens, one of 5..257 or <= 4 zeros
        any_byte       that grammar for stretches of six and more equal bytes of every value, wherever they lie
        threes, fours  such stretches cut into tokens of length 3 / 4 only
        tail_first     the remainder token in front of the 258s
        random_cuts    a seeded random split that uses every length symbol and every extra-bit count
        literals_only  no run tokens at all
    long258: every other 258 of the policy as symbol 284 + extra 31."""
    assert policy in UF_POLICIES
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    if policy == "literals_only" or a.size == 0:
        return [a.tobytes()] if a.size else []
    r = np.random.default_rng(seed)
    if policy == "reference":
        whole = a.size & ~7
        starts, ends = _stretches(a[:whole], True)
        keep = starts + ((7 - starts) % 8) < ends
        starts, ends = starts[keep], ends[keep]
    else:
        starts, ends = _stretches(a, False)
        keep = ends - starts >= 6
        starts, ends = starts[keep], ends[keep]
    toks, at, flip = [], 0, False
    for s, e in zip(starts.tolist(), ends.tolist()):
        cuts, lits = _cut_run(e - s - 1, policy, r)
        toks.append(a[at:s + 1].tobytes())
        for c in cuts:
            flip = not flip
            toks.append(M(c, 1, long258=long258 and c == 258 and flip))
        at = e - lits
    if at < a.size:
        toks.append(a[at:].tobytes())
    return toks


def token_stats(tokens):
    """-> dict(literals, matches, longest stretch of match tokens in a row, set of lengths)"""
    lit = mat = run = best = 0
    lengths = set()
    for t in tokens:
        if isinstance(t, tuple):
            mat += 1
            run += 1
            best = max(best, run)
            lengths.add(t[0])
        else:
            lit += len(t) if not isinstance(t, int) else 1
            run = 0
    return dict(literals=lit, matches=mat, chain=best, lengths=lengths)


# --------------------------------------------------------------------------------------
# the corpus
# --------------------------------------------------------------------------------------
def caps_for(raw_len):
    """the slots a valid stream is decoded into (the rule of tests/test_gpu_parity.py)"""
    return sorted(set([raw_len, raw_len + 1, raw_len + 777, max(raw_len - 1, 0), raw_len // 2, 0]))


RUN_LENGTHS = (5, 8, 257, 258, 259, 260, 516, 517, 1024, 1290, 258 * 5 + 1, 258 * 6 + 1, 258 * 64 + 1, 258 * 64 + 2,
               258 * 65 + 7)     # (that test's list names 1291 twice: as 1291 and as 258 * 5 + 1)
FLAT_RUNS = RUN_LENGTHS + (258 * 128 + 1, 40000)   # the zero runs of test_landing_decoder_flat_stretches


def _noisy(r, n):
    x = r.integers(0, 256, n, dtype=np.uint8)
    x[r.random(n) < 0.3] = 0
    return x


def _uf(tokens):
    """uf_foreign with the info of StreamWriter.done, and the longest stretch of run tokens in stream bits"""
    hl = constants()["HUFFMAN_LENGTHS"]
    best = cur = 0
    for t in tokens:
        if isinstance(t, tuple):
            ls = 27 if t[2] else _LEN_SYM[t[0]]
            cur += hl[257 + ls] + LEN_EXTRA[ls] + 1
            best = max(best, cur)
        else:
            cur = 0
    comp, raw = uf_foreign(tokens)
    return comp, raw, dict(chain_bits=best, data_bits=8 * (len(comp) - 4 - 53) - 5)


def _u_nonzero_run(add):
    """One run of a non-zero byte in a noisy buffer; the byte goes round (1, 0x80, 0xFF) over (length, place)."""
    r = np.random.default_rng(9101)
    k = 0
    for total in (20000, 65536):
        for run in RUN_LENGTHS:
            for at in (1, 8, 4097, total - run - 100, total - run):
                v = (1, 0x80, 0xFF)[k % 3]
                k += 1
                x = _noisy(r, total)
                x[at:at + run] = v
                if at:
                    x[at - 1] = v ^ 0x55          # the run starts where it is put
                toks = uf_parse(x, "any_byte")
                assert any(isinstance(t, tuple) for t in toks)
                add("U_nonzero_run", "t%d_r%d_a%d_v%d" % (total, run, at, v), *_uf(toks))


def _u_lanes(add):
    """Streams the segment kernel takes (8 KiB compressed and more) with non-zero runs so long that several lanes'
    bit ranges hold run tokens only."""
    r = np.random.default_rng(9102)
    for run, v in ((30000, 0x41), (100000, 0xFF), (200000, 0x80)):
        x = _noisy(r, 12000 + run + 9000)
        x[12000:12000 + run] = v
        x[11999] = v ^ 1
        add("U_lanes_without_literals", "run%d" % run, *_uf(uf_parse(x, "any_byte")))
    x = _noisy(r, 10000 + 30000 + 1 + 40000 + 10000)
    x[10000:40000] = 0x33
    x[40000] = 0x77                                   # a single literal between two runs of different bytes
    x[40001:80001] = 0xCC
    add("U_lanes_without_literals", "two_runs", *_uf(uf_parse(x, "any_byte")))
    add("U_lanes_without_literals", "two_runs_fours", *_uf(uf_parse(x, "fours")))


def flat_buffers():
    """The zero-run buffers of test_landing_decoder_flat_stretches at one total, 65 536 -> list of (name, array)."""
    r = np.random.default_rng(606)
    total, out = 65536, []
    for run in FLAT_RUNS:
        if run + 200 > total:
            continue
        for at in (0, 1, 8, 4097, total - run - 100, total - run):
            x = _noisy(r, total)
            x[at:at + run] = 0
            out.append(("r%d_a%d" % (run, at), x))
    x = _noisy(r, total)
    for k in range(0, total - 2048, 2048):
        x[k + 1024:k + 2048] = 0
    out.append(("half", x))
    y = np.zeros(total, dtype=np.uint8)
    y[::1033] = 7
    out.append(("sparse7", y))
    out.append(("zeros", np.zeros(total, dtype=np.uint8)))
    return out


OFFGRAMMAR_POLICIES = ("threes", "fours", "tail_first", "random_cuts", "literals_only")


def _u_offgrammar(add):
    """Zero runs written off the encoder's grammar.  Every buffer under three of the five policies, the policies going
    round (all five on every buffer would be 36 MiB of payload; see the budget in corpus())."""
    for k, (name, x) in enumerate(flat_buffers()):
        for j in range(3):
            pol = OFFGRAMMAR_POLICIES[(k + 2 * j) % 5]
            add("U_offgrammar_zero", "%s_%s" % (name, pol), *_uf(uf_parse(x, pol, seed=k, long258=(k % 2 == 1))))
    r = np.random.default_rng(9103)
    head, tail = _noisy(r, 3000).tobytes() + b"\x09", b"\x0b" + _noisy(r, 3000).tobytes()
    # a chain of more than 64 tokens none of which is a 258
    toks = [head, b"\x00"] + [M(3 + (i * 37) % 254, 1) for i in range(200)] + [tail]
    add("U_offgrammar_zero", "chain200_non258", *_uf(toks))
    # a chain of 258s broken by a single zero literal
    toks = [head, b"\x00"] + [M(258, 1)] * 40 + [b"\x00"] + [M(258, 1)] * 70 + [b"\x00"] + [M(258, 1)] * 3 + [tail]
    add("U_offgrammar_zero", "chain258_broken", *_uf(toks))


def _u_all_symbols(add):
    r = np.random.default_rng(9104)
    toks = []
    lits = list(range(256))
    for i in range(29):
        for e in sorted(set((0, (1 << LEN_EXTRA[i]) - 1))):
            v = lits[(i * 9 + e) % 256]
            toks += [bytes(r.integers(0, 256, 3, dtype=np.uint8)), bytes([v]), M(min(LEN_BASE[i] + e, 258), 1)]
    toks += [bytes(r.permutation(256).astype(np.uint8)), bytes([0xEE]), M(258, 1, long258=True), bytes(range(255, -1, -1))]
    add("U_all_symbols", "all", *_uf(toks))


def _flat_lit(r=None):
    """a complete literal/length code over all 286 symbols, 8 and 9 bits"""
    return [8] * 226 + [9] * 60


def _g_overlap_grid(add):
    r = np.random.default_rng(9201)
    pairs = [(ln, d) for ln in range(3, 259) for d in range(1, ln + 1)]
    order = r.permutation(len(pairs))
    dist_l = spread(complete_code(17, 6, r, deep=0.2), list(range(17)), r, 30)   # distances up to 258: symbols 0..16
    lit_l = spread(complete_code(286, 11, r, deep=0.1), list(range(286)), r, 286)

    def head():
        return [bytes(r.integers(0, 256, 258, dtype=np.uint8))], 258     # room for every distance from the first match on

    (toks, size), part = head(), 0
    for k in order.tolist() + [None]:
        if k is not None:
            nl = int(r.integers(1, 5))
            toks += [bytes(r.integers(0, 256, nl, dtype=np.uint8)), M(*pairs[k])]
            size += nl + pairs[k][0]
        if (k is None and len(toks) > 1) or size >= 65536:
            add("G_overlap_grid", "p%02d_fixed" % part, *StreamWriter().fixed(toks, final=True).done())
            add("G_overlap_grid", "p%02d_dyn" % part, *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r).done())
            (toks, size), part = head(), part + 1


RING_LENS = (3, 4, 8, 12, 13, 16, 17, 63, 64, 65, 257, 258)
RING_DISTS = (255, 256, 257, 2047, 2048, 2049, 3327, 3328, 3329, 3583, 3584, 3585, 32767, 32768)


def _g_ring_edges(add):
    r = np.random.default_rng(9202)
    pairs = []
    for ln in RING_LENS:
        for d in sorted(set((ln, ln + 1) + RING_DISTS)):
            pairs.append((ln, d))
    body = [bytes(r.integers(0, 256, 32768, dtype=np.uint8))]
    for k in r.permutation(len(pairs)).tolist():
        body += [M(*pairs[k]), bytes(r.integers(0, 256, int(r.integers(1, 4)), dtype=np.uint8))]
    lit_l = spread(complete_code(286, 10, r, deep=0.05), list(range(286)), r, 286)
    dist_l = spread(complete_code(30, 7, r, deep=0.1), list(range(30)), r, 30)
    for phase in range(64):
        toks = [bytes(r.integers(0, 256, phase, dtype=np.uint8))] + body if phase else body
        sw = StreamWriter()
        if phase % 2:
            sw.fixed(toks, final=True)
        else:
            sw.dynamic(toks, lit_l, dist_l, final=True, r=r)
        add("G_ring_edges", "phase%02d" % phase, *sw.done())


WINDOW_STARTS = (1, 2, 3, 15, 16, 17, 255, 256, 257, 3584, 32767, 32768)


def _g_window_start(add):
    r = np.random.default_rng(9203)
    for opos in WINDOW_STARTS:
        for ln in (3, 258):
            toks = [bytes(r.integers(0, 256, opos, dtype=np.uint8)), M(ln, opos), bytes(r.integers(0, 256, 5, dtype=np.uint8)),
                    M(9, opos + ln + 5 if opos + ln + 5 <= 32768 else 7)]
            add("G_window_start", "o%d_l%d" % (opos, ln), *StreamWriter().fixed(toks, final=True).done())


def _g_dense(add):
    r = np.random.default_rng(9204)
    seed = bytes(r.integers(0, 256, 8, dtype=np.uint8))
    vals = sorted(set(seed))
    # symbol 257 (length 3): one bit; the seed's literals and the end-of-block share the other half
    lit_l = [0] * 286
    lit_l[257] = 1
    for s, l in zip(vals + [256], complete_code(len(vals) + 1, 6, r, deep=0.2)):
        lit_l[s] = l + 1
    dist_l = [1, 2, 3, 0, 0, 3]          # distances 1, 2, 3 and 7..8 (one extra bit)
    for name, ds in (("d1", (1,)), ("d2", (2,)), ("d3", (3,)), ("d7", (7,)), ("mixed", (1, 2, 3, 7))):
        toks = [seed] + [M(3, ds[int(r.integers(0, len(ds)))]) for _ in range(6000)]
        add("G_dense_matches", name, *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r).done())


def _g_expansion(add):
    r = np.random.default_rng(9205)
    lit_l = [9] * 255 + [10, 10] + [0] * 29      # 255 x 9 bits + 2 x 10 bits (literal 255, end-of-block): one half
    lit_l[285] = 1                                # length 258: one bit
    for d in (1, 2, 3, 7, 255, 258, 3000):
        dist_l = [0] * 30
        dist_l[dist_symbol(d)] = 1
        toks = [bytes(r.integers(0, 256, 3000, dtype=np.uint8))] + [M(258, d)] * 400
        add("G_expansion", "d%d" % d, *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r).done())
    dist_l = [2, 2, 2, 0, 0, 2]                   # two-bit distance codes, the distances mixed
    toks = [bytes(r.integers(0, 256, 3000, dtype=np.uint8))] + [M(258, (1, 2, 3, 7)[int(r.integers(0, 4))]) for _ in range(400)]
    add("G_expansion", "mixed", *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r).done())


def _g_long_tokens(add):
    r = np.random.default_rng(9206)
    # literals 0..253 and the end-of-block at 8 bits; under the last 8-bit prefix a chain 9, 10, .., 15, 15 whose two
    # 15-bit codes are the length symbols 281 and 284 (five extra bits each)
    lit_l = [8] * 254 + [9, 10, 8, 11, 12, 13, 14] + [0] * 25
    lit_l[281] = lit_l[284] = 15
    dist_l = list(range(1, 15)) + [0] * 14 + [15, 15]     # symbols 28 and 29: 15 bits + 13 extra bits
    toks = [bytes(r.integers(0, 254, 32768, dtype=np.uint8))]
    for _ in range(500):
        ls = (24, 27)[int(r.integers(0, 2))]
        ln = LEN_BASE[ls] + int(r.integers(0, 32))
        toks.append(M(min(ln, 257), int(r.integers(16385, 32769))))
    sw = StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r)
    add("G_long_tokens", "tok48", *sw.done())
    # every literal at 13..15 bits: 32 x 13 + 160 x 14 + 64 x 15 = 2^-6; EOB, 257..261 at 1..6 bits
    lens = [13] * 32 + [14] * 160 + [15] * 64
    lit_l = spread(lens, list(range(256)), r, 286)
    for s, l in zip((256, 257, 258, 259, 260, 261), (1, 2, 3, 4, 5, 6)):
        lit_l[s] = l
    toks = []
    for _ in range(60):
        toks += [bytes(r.integers(0, 256, 40, dtype=np.uint8)), M(int(r.integers(3, 8)), int(r.integers(1, 30)))]
    dist_l = spread(complete_code(10, 5, r), list(range(10)), r, 30)
    add("G_long_tokens", "deep_literals", *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, r=r).done())


def table_class_codes(lit_bits, dist_bits, sub, dsub):
    """-> {("lit" | "dist", class): code lengths over all 286 / 30 symbols} for every class that exists"""
    r = np.random.default_rng(9207)
    out = {}
    for cls in TABLE_CLASSES:
        for which, n, bits, cap in (("lit", 286, lit_bits, sub), ("dist", 30, dist_bits, dsub)):
            lens = code_of_class(cls, n, bits, cap, r)
            if lens is not None:
                out[(which, cls)] = spread(lens, list(range(n)), r, n)
    return out


LZ_CONSTANTS = dict(lit_bits=9, dist_bits=8, sub=256, dsub=64)   # inflate_lz.h; tests/test_deflate_gen.py reads the header


def _g_table_classes(add):
    r = np.random.default_rng(9208)
    codes = table_class_codes(**LZ_CONSTANTS)
    plain_dist = spread(complete_code(30, 7, r, deep=0.1), list(range(30)), r, 30)
    for (which, cls), lens in sorted(codes.items()):
        if which == "lit":
            # every literal, every length symbol at its lowest and highest extra value
            toks = [bytes(r.permutation(256).astype(np.uint8))]
            for i in range(29):
                for e in sorted(set((0, (1 << LEN_EXTRA[i]) - 1))):
                    ln = min(LEN_BASE[i] + e, 258)
                    toks += [M(ln, int(r.integers(1, 200))), bytes(r.integers(0, 256, 2, dtype=np.uint8))]
            toks.append(bytes(r.permutation(256).astype(np.uint8)))
            sw = StreamWriter().dynamic(toks, lens, plain_dist, final=True, r=r)
        else:
            toks = [bytes(r.integers(0, 256, 32768, dtype=np.uint8))]
            for rep in range(2):
                for s in r.permutation(30).tolist():
                    d = DIST_BASE[s] + int(r.integers(0, 1 << DIST_EXTRA[s]))
                    toks += [M(int(r.integers(3, 40)), d), bytes(r.integers(0, 256, 2, dtype=np.uint8))]
            sw = StreamWriter().dynamic(toks, _flat_lit(), lens, final=True, r=r)
        add("G_table_classes", "%s_%s" % (which, cls), *sw.done())


def hclen_lengths(k):
    """A complete literal/length code whose lengths need exactly the first k entries of the code-length order (k in
    5..19; with k = 4 only length 0 can be written, which is no code): 8-bit codes, some merged into one shorter code
    or one split into longer ones, so that length CLCL_ORDER[k - 1] is used and no length behind it."""
    allowed = [l for l in CLCL_ORDER[3:k] if l]
    L = CLCL_ORDER[k - 1]
    assert 8 in allowed
    lens = [8] * 256
    if L < 8:
        del lens[:1 << (8 - L)]
        lens.append(L)
    elif L > 8:
        need = (1 << (L - 8)) - 1
        shorter = sorted(l for l in allowed if l < 8)
        while len(lens) + need > 285:
            m = shorter[0]
            del lens[:1 << (8 - m)]
            lens.append(m)
        lens.remove(8)
        lens += [L] * (need + 1)
    assert kraft(lens) == 32768 and set(lens) <= set(allowed) and L in lens
    lens.sort()
    # symbol 256 gets the first length, symbol 0 none (a zero length in front: two code-length symbols at the least)
    out = [0] * 286
    out[256] = lens[0]
    for s, l in zip(range(1, 256), lens[1:]):
        out[s] = l
    for s, l in zip(range(257, 286), lens[256:]):
        out[s] = l
    assert sum(1 for l in out if l) == len(lens)
    return out


def _plain_syms(seq):
    return [(l, 0) for l in seq]


def _g_headers(add):
    r = np.random.default_rng(9209)
    # ---- HCLEN 5..19, each exactly what its code-length code needs (4: see hclen_lengths) ----
    for k in range(5, 20):
        lit_l = hclen_lengths(k)
        usable = np.array([s for s in range(256) if lit_l[s]], dtype=np.uint8)
        toks = [usable.tobytes(), r.choice(usable, 300).astype(np.uint8).tobytes()]
        seq = lit_l[:max(257, max(s + 1 for s in range(286) if lit_l[s]))] + [0]
        syms = _plain_syms(seq)
        cl = cl_code_for(syms, r)
        need = max(i + 1 for i in range(19) if cl[CLCL_ORDER[i]])
        assert need == k, (k, need)
        sw = StreamWriter().dynamic(toks, lit_l, [0], final=True, cl_syms=syms, cl_lengths=cl, r=r)
        add("G_headers", "hclen%d" % k, *sw.done())
        if k < 19:   # the same block with HCLEN one more than needed (a trailing zero in the code-length code's lengths)
            sw = StreamWriter().dynamic(toks, lit_l, [0], final=True, cl_syms=syms, cl_lengths=cl, hclen=k + 1, r=r)
            add("G_headers", "hclen%d_padded" % k, *sw.done())
    # ---- HLIT x HDIST, the last length of each used or zero ----
    for hlit in (257, 258, 285, 286):
        for hdist in (1, 2, 29, 30):
            for trailing in (False, True):
                nl = hlit - (3 if trailing and hlit > 258 else 0) if hlit > 258 else hlit
                nd = hdist - (2 if trailing and hdist > 2 else 0)
                if trailing and hlit <= 258 and hdist <= 2:
                    continue      # nothing to leave zero: 256 needs its code, and so does the one distance
                nlit = nl if not (trailing and hlit == 258) else 257
                lit_l = spread(complete_code(nlit, 11, r, deep=0.1), list(range(nlit)), r, 286)
                if nd == 1:
                    dist_l = [1]
                else:
                    dist_l = spread(complete_code(nd, 9, r, deep=0.3), list(range(nd)), r, 30)
                if trailing and hdist <= 2:
                    dist_l = [1]
                toks = [bytes(r.integers(0, 256, 300, dtype=np.uint8))]
                top_l = max(s for s in range(257, 286) if lit_l[s]) - 257 if nlit > 257 else None
                top_d = max(s for s in range(30) if s < len(dist_l) and dist_l[s])
                for j in range(12):
                    if top_l is None:
                        break
                    ls = top_l if j % 3 == 0 else int(r.integers(0, top_l + 1))
                    ds = top_d if j % 4 == 0 else int(r.integers(0, top_d + 1))
                    d = DIST_BASE[ds] + int(r.integers(0, 1 << DIST_EXTRA[ds]))
                    if d > 300 + j * 4:
                        d = DIST_BASE[0] + 0 if dist_l[0] else None
                    if d is None or not dist_l[dist_symbol(d)]:
                        continue
                    toks += [M(min(LEN_BASE[ls], 258), d), bytes(r.integers(0, 256, 2, dtype=np.uint8))]
                sw = StreamWriter().dynamic(toks, lit_l, dist_l, final=True, hlit=hlit, hdist=hdist, r=r)
                add("G_headers", "hlit%d_hdist%d%s" % (hlit, hdist, "_zeros" if trailing else ""), *sw.done())
    # ---- every repeat count: one block each; 16 x 3..6, 17 x 3..10, 18 x 11..138 ----
    sw = StreamWriter()
    for sym, counts in ((16, range(3, 7)), (17, range(3, 11)), (18, range(11, 139))):
        for c in counts:
            if sym == 16:
                # 1 + c equal lengths of 3 among eight 3-bit codes: the literals 65.. and the end-of-block
                lit_l = [0] * 257
                for s in range(65, 72):
                    lit_l[s] = 3
                lit_l[256] = 3
                seq = lit_l + [0]
                syms = _plain_syms(seq[:65]) + [(3, 0), (16, c - 3)] + _plain_syms(seq[66 + c:])
                toks = [bytes(r.integers(65, 72, 30, dtype=np.uint8))]
            else:
                # a stretch of exactly c zero lengths in front of literal 200, written as one repeat; 256 literals less
                # the stretch share a complete code with the end-of-block
                used = [s for s in range(256) if not (200 - c <= s < 200)] + [256]
                lit_l = spread(complete_code(len(used), 12, r, deep=0.05), used, r, 257)
                seq = lit_l + [0]
                syms = _plain_syms(seq[:200 - c]) + [(sym, c - (3 if sym == 17 else 11))] + _plain_syms(seq[200:])
                toks = [r.choice(np.array(used[:-1], dtype=np.uint8), 40).astype(np.uint8).tobytes()]
            sw.dynamic(toks, lit_l, [0], cl_syms=syms, r=r)
    sw.fixed([], final=True)
    add("G_headers", "every_repeat", *sw.done())
    # ---- runs across the literal/distance boundary ----
    lit_l = [8] * 191 + [0] * 65 + [8] + [0] * 27 + [3, 3]        # 192 x 8 bits + 284, 285 at 3 bits
    dist_l = [3] * 8
    seq = lit_l + dist_l
    syms = rle_lengths(seq[:284]) + [(3, 0), (16, 3), (16, 0)]      # 3, then 6 + 3 repeats: 285 and all eight distances
    toks = [bytes(r.integers(0, 191, 200, dtype=np.uint8)), M(258, 5), M(227, 8), bytes(r.integers(0, 191, 9, dtype=np.uint8))]
    add("G_headers", "equal_run_across", *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, cl_syms=syms, r=r).done())
    lit_l = spread(complete_code(276, 11, r, deep=0.1), list(range(276)), r, 276)   # 276..285 zero, HLIT 286
    dist_l = [0, 0, 0, 1, 1]
    seq = lit_l + [0] * 10 + dist_l
    for sym, extra, lead, nm in ((17, 7, [(0, 0)] * 3, "17"), (18, 2, [], "18")):
        # 13 zeros, ten literal/length and three distance: three plain and one repeat of 10, or one repeat of 13
        assert len(lead) + (3 + extra if sym == 17 else 11 + extra) == 13
        syms = rle_lengths(seq[:276], use17=False, use18=False) + lead + [(sym, extra)] + [(1, 0), (1, 0)]
        toks = [bytes(r.integers(0, 256, 100, dtype=np.uint8)), M(12, 4), bytes([7]), M(30, 6)]
        add("G_headers", "zero_run_across_" + nm, *StreamWriter().dynamic(toks, lit_l, dist_l, final=True, hlit=286,
                                                                             cl_syms=syms, r=r).done())
    # ---- one distance code, at symbol 0, 4 and 29 (13 extra bits) ----
    for ds in (0, 4, 29):
        dist_l = [0] * 30
        dist_l[ds] = 1
        toks = [bytes(r.integers(0, 256, 32768 if ds == 29 else 64, dtype=np.uint8))]
        for _ in range(40):
            d = DIST_BASE[ds] + int(r.integers(0, 1 << DIST_EXTRA[ds]))
            toks += [M(int(r.integers(3, 259)), d), bytes(r.integers(0, 256, 1, dtype=np.uint8))]
        add("G_headers", "one_dist_sym%d" % ds, *StreamWriter().dynamic(toks, _flat_lit(), dist_l, final=True, r=r).done())


BLOCK_KINDS = ("stored", "fixed", "dynamic", "empty_dynamic", "empty_fixed", "empty_stored")
EMPTY_DYN = [0] * 256 + [1, 1]          # end-of-block and one length symbol, one bit each; no distance code


def _g_block_mix(add):
    for seed, last in ((9210, "empty_fixed"), (9211, "empty_stored"), (9215, "empty_dynamic")):
        r = np.random.default_rng(seed)
        sw = StreamWriter()
        starts = []                                   # payload position at which each block with payload starts
        for i in range(300):
            # the kinds go round, forwards and backwards in turn: a stored header then follows every other kind
            rnd, j = divmod(i, 6)
            kind = BLOCK_KINDS[j if rnd % 2 == 0 else 5 - j]
            n = int(r.integers(20, 61))
            if kind == "stored":
                starts.append(len(sw.out))
                sw.stored(bytes(r.integers(0, 256, n, dtype=np.uint8)))
            elif kind in ("fixed", "dynamic"):
                here = len(sw.out)
                toks = [bytes(r.integers(0, 256, max(n - 12, 4), dtype=np.uint8))]
                if starts:
                    back = starts[-min(len(starts), int(r.integers(1, 4)))]     # 1..3 blocks back
                    d = here + len(toks[0]) - back - int(r.integers(0, 8))
                    toks += [M(int(r.integers(3, 13)), max(d, 1))]
                toks.append(bytes(r.integers(0, 256, 2, dtype=np.uint8)))
                starts.append(here)
                if kind == "fixed":
                    sw.fixed(toks)
                else:
                    lit_l = spread(complete_code(286, 12, r, deep=0.1), list(range(286)), r, 286)
                    dist_l = spread(complete_code(30, 8, r, deep=0.1), list(range(30)), r, 30)
                    sw.dynamic(toks, lit_l, dist_l, r=r)
            elif kind == "empty_dynamic":
                sw.dynamic([], EMPTY_DYN, [0], r=r)
            elif kind == "empty_fixed":
                sw.fixed([])
            else:
                sw.stored(b"")
        if last == "empty_fixed":
            sw.fixed([], final=True)
        elif last == "empty_stored":
            sw.stored(b"", final=True)
        else:
            sw.dynamic([], EMPTY_DYN, [0], final=True, r=r)
        add("G_block_mix", "mix300_" + last, *sw.done())
    # matches that reach back into, and over the edges of, bytes a stored block delivered
    r = np.random.default_rng(9213)
    lit_l = spread(complete_code(286, 10, r, deep=0.05), list(range(286)), r, 286)
    dist_l = spread(complete_code(30, 6, r, deep=0.05), list(range(30)), r, 30)
    for name, nstored, dists in (("stored65535", 65535, lambda: int(r.integers(30000, 32769))),
                                 ("stored20000", 20000, lambda: int(r.choice([r.integers(19700, 20300), r.integers(30000, 32769)])))):
        sw = StreamWriter()
        sw.dynamic([bytes(r.integers(0, 256, 40000, dtype=np.uint8))], lit_l, dist_l, r=r)
        sw.stored(bytes(r.integers(0, 256, nstored, dtype=np.uint8)))
        toks = []
        for _ in range(600):
            toks += [M(int(r.integers(3, 259)), dists()), bytes(r.integers(0, 256, int(r.integers(1, 3)), dtype=np.uint8))]
        sw.fixed(toks[:600])
        sw.dynamic(toks[600:], lit_l, dist_l, final=True, r=r)
        add("G_block_mix", name, *sw.done())


_BUILDERS = (_u_nonzero_run, _u_lanes, _u_offgrammar, _u_all_symbols, _g_overlap_grid, _g_ring_edges, _g_window_start,
             _g_dense, _g_expansion, _g_long_tokens, _g_table_classes, _g_headers, _g_block_mix)
CLASSES = ("U_nonzero_run", "U_lanes_without_literals", "U_offgrammar_zero", "U_all_symbols", "G_overlap_grid",
           "G_ring_edges", "G_window_start", "G_dense_matches", "G_expansion", "G_long_tokens", "G_table_classes",
           "G_headers", "G_block_mix")
MAX_PAYLOAD = 48 << 20
MAX_CORE = 2 << 20

_cache = {}


def corpus():
    """-> list of (class, name, stream, payload), cached per process.  At most 48 MiB of payload in all."""
    if "corpus" not in _cache:
        rows, info = [], {}

        def add(cls, name, comp, raw, info_):
            rows.append((cls, name, bytes(comp), bytes(raw)))
            info[(cls, name)] = info_

        for b in _BUILDERS:
            b(add)
        assert sum(len(x[3]) for x in rows) <= MAX_PAYLOAD
        assert len(set((c, n) for c, n, _, _ in rows)) == len(rows)
        _cache["corpus"], _cache["info"] = rows, info
    return _cache["corpus"]


def corpus_info():
    """-> {(class, name): what the writer recorded about a stream (StreamWriter.done, _uf)}"""
    corpus()
    return _cache["info"]


def core():
    """The two smallest streams of every class (three where they are tiny): at most 2 MiB of payload, for the runs
    that repeat over many flag sets."""
    if "core" not in _cache:
        out = []
        for cls in CLASSES:
            rows = sorted((x for x in corpus() if x[0] == cls), key=lambda x: (len(x[3]), x[1]))
            out += rows[:3 if sum(len(x[3]) for x in rows[:3]) <= 100000 else 2]
        assert sum(len(x[3]) for x in out) <= MAX_CORE
        _cache["core"] = out
    return _cache["core"]


def error_corpus():
    """-> list of (class, name, stream, expected status name or None where only parity with the oracle counts)"""
    if "errors" in _cache:
        return _cache["errors"]
    r = np.random.default_rng(9301)
    out = []
    noise = _noisy(r, 3000).tobytes()
    # a run token as the very first token of an ultra-fast stream; the distance bit set
    first = uf_foreign([M(258, 1), noise], lenient=True)[0]
    out.append(("U_errors", "run_first", first, "DistanceTooFarBack"))
    bad_bit = uf_foreign([noise, b"\x05", M(100, 1, dbits=(1, 1)), noise])[0]
    out.append(("U_errors", "distance_bit_set", bad_bit, "InvalidDistanceCode"))
    for nm, s in (("run_first", first), ("distance_bit_set", bad_bit)):
        for cut in (54, 60, len(s) // 2):
            out.append(("U_errors", "%s_cut%d" % (nm, cut), s[:cut], None))
    # a match that starts one byte in front of the output
    for opos in WINDOW_STARTS:
        if opos + 1 > 32768:
            continue
        sw = StreamWriter()
        sw.lenient = True
        sw.fixed([bytes(r.integers(0, 256, opos, dtype=np.uint8))])
        sw.fixed([M(3, opos + 1), b"ab"], final=True)
        out.append(("G_window_start", "o%d_too_far" % opos, sw.finish()[0], "DistanceTooFarBack"))
    _cache["errors"] = out
    return out


def truncations():
    """Of the first stream of 400 bytes or more of every class: cuts at 24 seeded places and at the last 12 bytes -> list of (name, bytes)"""
    import random
    rnd = random.Random(77)
    out = []
    for cls in CLASSES:
        rows = [x for x in corpus() if x[0] == cls]
        _, name, comp, _ = next((x for x in rows if len(x[2]) >= 400), rows[-1])
        cuts = sorted(set([rnd.randrange(2, len(comp)) for _ in range(24)] + list(range(len(comp) - 12, len(comp)))))
        out += [("%s/%s_cut%d" % (cls, name, c), comp[:c]) for c in cuts]
    return out


def class_digests():
    """-> {class: SHA-256 over its streams in corpus order}; error_corpus and truncations under their own names"""
    h = {}
    for cls, _, comp, _ in corpus():
        h.setdefault(cls, hashlib.sha256()).update(len(comp).to_bytes(8, "little") + comp)
    for key, rows in (("errors", [x[2] for x in error_corpus()]), ("truncations", [x[1] for x in truncations()])):
        d = hashlib.sha256()
        for comp in rows:
            d.update(len(comp).to_bytes(8, "little") + comp)
        h[key] = d
    return {k: v.hexdigest() for k, v in h.items()}


# --------------------------------------------------------------------------------------
# random streams (tests/soak_gpu.py)
# --------------------------------------------------------------------------------------
def random_general(r, size=20000):
    """A random multi-block stream: random complete codes up to 15 bits, random tokens."""
    sw = StreamWriter()
    nblocks = int(r.integers(1, 6))
    for b in range(nblocks):
        final = b == nblocks - 1
        kind = int(r.integers(0, 4))
        n = int(r.integers(0, size // nblocks + 1))
        if kind == 0:
            sw.stored(bytes(r.integers(0, 256, min(n, 65535), dtype=np.uint8)), final=final)
            continue
        toks, made = [], 0
        while made < n:
            k = int(r.integers(1, 30))
            toks.append(bytes(r.integers(0, 256, k, dtype=np.uint8)))
            made += k
            if len(sw.out) + made > 0 and r.random() < 0.7:
                ln = int(r.integers(3, 259))
                d = int(min(np.exp(r.uniform(0, np.log(32768.0))), len(sw.out) + made, 32768))
                toks.append(M(ln, max(d, 1)))
                made += ln
        if kind == 1:
            sw.fixed(toks, final=final)
        else:
            lit_l = spread(complete_code(286, int(r.integers(9, 16)), r, deep=float(r.random()) * 0.5), list(range(286)), r, 286)
            dist_l = spread(complete_code(30, int(r.integers(5, 16)), r, deep=float(r.random())), list(range(30)), r, 30)
            sw.dynamic(toks, lit_l, dist_l, final=final, r=r)
    return sw.finish()


def random_uf(r, size=60000):
    """A random buffer with runs of random bytes, under a random policy, behind the ultra-fast prefix."""
    n = int(r.integers(0, size))
    x = _noisy(r, n)
    for _ in range(int(r.integers(0, 8))):
        if n:
            lo = int(r.integers(0, n))
            x[lo:lo + int(np.exp(r.uniform(1, np.log(40000.0))))] = int(r.integers(0, 256)) if r.random() < 0.7 else 0
    pol = UF_POLICIES[int(r.integers(1, len(UF_POLICIES)))]
    return uf_foreign(uf_parse(x, pol, seed=int(r.integers(0, 1 << 30)), long258=bool(r.integers(0, 2))))
