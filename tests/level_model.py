"""Pure-Python restatement of the reference's general encoder for levels 1, 2 and 3 and RLE: whole zlib
streams, no compiled code.

The expected bytes of levels 2 and 3 in the GPU tests of those levels come from here.  tests/test_level_model.py pins
this model against the oracle (oracle/fdeflate_oracle.c) at level 1 and RLE over the oracle tests' encoder inputs and
the run-edge inputs: that pins the parser, the runs, match_length::<true>, block cutting and the whole block writer.
HashChainMatchFinder (hashchain.rs) and match_length::<false> (matchfinder/mod.rs:71-76), about 150 lines here
(`Chain`, and the `min8 = False` branch of `match_length`), are stated a second time in the oracle's C
(fdo_compress_level, written from the Rust apart from this file); tests/test_oracle_levels.py holds the two readings
to the same bytes and the same counts of the finder's exits.  The real crate cannot be run here.

Reference: Compressor::write_data + finish for one buffer (src/compress/mod.rs:126-214), ParserInner
(parse/mod.rs), GreedyParser (parse/greedy.rs), RleParser (parse/rle.rs), HashTableMatchFinder
(matchfinder/hashtable.rs), HashChainMatchFinder (matchfinder/hashchain.rs), match_length / rle_match
(matchfinder/mod.rs), write_block / build_huffman_tree (bitstream.rs:41-325; the order of Rust's
BinaryHeap as restated in oracle/fdeflate_oracle.c).

`compress(data, level)` and `compress_rle(data)` return the stream; the counters of the chain search of
the last call are in `last_counters` (a dict, empty for level 1 and RLE):
  steps2    candidates visited beyond the first of a walk
  nice      walks ended by length >= nice_length
  eod       walks ended by ip + length == len(data)
  depth     walks ended by search_depth
  alias     visits of a candidate at exactly ip - 32768 (its link slot was just overwritten)
  unwritten reads of a link slot never written in this stream
  maxsteps  the longest walk
and `last_exits` counts, for the last call at any level, how the device's counter of equal bytes (equal_bytes in
deflate_general.hip) would have ended each of its calls: (use, exit) -> calls, see `_note_exit`.
"""
import bisect
import collections
import functools
import zlib

import numpy as np

M64 = (1 << 64) - 1
W = 32768
CACHE = 65536
BLOCK_SYMBOLS = 16384

# RFC 1951 tables (reference src/tables.rs, data)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLCL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LENGTH_TO_SYMBOL = [0] * 256   # length - 3 -> symbol
LENGTH_TO_EXTRA = [0] * 256
for _s in range(28):
    for _l in range(LEN_BASE[_s], LEN_BASE[_s + 1]):
        LENGTH_TO_SYMBOL[_l - 3] = 257 + _s
        LENGTH_TO_EXTRA[_l - 3] = LEN_EXTRA[_s]
LENGTH_TO_SYMBOL[255] = 285     # 258 has a symbol of its own

last_counters = {}
last_exits = collections.Counter()
_exits = collections.Counter()      # of the call that is running

USES = ("match_back", "match_fwd", "run_back", "run_fwd")       # the walks from a match / inside a run, either way
EXITS = ("group32", "group8", "wide", "bytes", "limit")


def _note_exit(use, limit, n, room):
    """The device counts equal bytes 32 at a time (four loads in flight), then 8 at a time, then takes a tail shorter
    than 8 with one wide load where 8 bytes are readable (`room`: the bytes readable in the walking direction), byte
    by byte where not.  A call that may test `limit` bytes and finds n equal ends at the limit, or at a difference
    inside a group of 32, a group of 8, the wide tail or the byte tail.  A call with nothing to test is not counted."""
    assert 0 <= n <= limit <= room, (use, limit, n, room)
    if limit == 0:
        return
    whole = limit - limit % 8
    if n == limit:
        e = "limit"
    elif n < whole:
        e = "group32" if n < limit - limit % 32 else "group8"
    else:
        e = "wide" if whole + 8 <= room else "bytes"
    _exits[use, e] += 1


def ld64(d, i):
    return int.from_bytes(d[i:i + 8], "little")


def chash(v):
    return ((11400714785074694791 * v) & M64) >> 40


def _tz8(x):
    return ((x & -x).bit_length() - 1) // 8


def _equal_fwd(data, a, b, limit):
    """Number of i < limit with data[a + i] == data[b + i] for all smaller i as well."""
    if limit <= 0:
        return 0
    x = int.from_bytes(data[a:a + limit], "little") ^ int.from_bytes(data[b:b + limit], "little")
    return limit if x == 0 else _tz8(x)


def _equal_back(data, a_end, b_end, limit):
    """Number of i < limit with data[a_end - 1 - i] == data[b_end - 1 - i] for all smaller i as well."""
    if limit <= 0:
        return 0
    x = int.from_bytes(data[a_end - limit:a_end], "big") ^ int.from_bytes(data[b_end - limit:b_end], "big")
    return limit if x == 0 else _tz8(x)


def match_length(min8, value, data, anchor, ip, prev):
    """matchfinder/mod.rs:51-110."""
    assert prev < ip
    assert prev + 8 <= len(data)
    pv = ld64(data, prev)
    if min8:
        if value != pv:
            return 0, ip
        length = 8
    else:
        if (value & 0xFFFFFFFF) != (pv & 0xFFFFFFFF):
            return 0, ip
        x = value ^ pv
        length = 8 if x == 0 else _tz8(x)      # u64::trailing_zeros of 0 is 64
    # while length < 258 && ip > anchor && prev_index > 0 && data[ip - 1] == data[prev_index - 1]
    first8 = length == 8
    lim = min(258 - length, ip - anchor, prev)
    n = _equal_back(data, ip, prev, lim)
    _note_exit("match_back", lim, n, prev)
    length += n
    ip -= n
    prev -= n
    # chunks of 8, then the remainder byte by byte: the count of equal bytes either way
    sl = min(len(data) - ip - length, 258 - length)
    k = _equal_fwd(data, ip + length, prev + length, sl)
    if first8:      # (fewer than 8: the next byte is the one that differed, the device does not look)
        _note_exit("match_fwd", sl, k, len(data) - ip - length)
    return length + k, ip


def rle_match(data, last_match, ip):
    """matchfinder/mod.rs:113-145."""
    value = data[ip]
    start, length = ip + 1, 4
    min_start = max(1, last_match, max(0, start + length - 258))
    while start > min_start and data[start - 2] == value:
        start -= 1
        length += 1
    _note_exit("run_back", max(ip + 1 - min_start, 0), length - 4, ip)
    e = start + length
    lim = min(len(data) - e, 258 - length)
    run = data[e:e + lim]
    k = len(run) - len(run.lstrip(bytes([value]))) if lim > 0 else 0
    _note_exit("run_fwd", lim, k, len(data) - e)
    return [length + k, 1, start]


class Null:
    c = {}

    def get_and_insert(self, data, base, anchor, ip, value):
        return [0, 0, 0]

    def insert(self, value, off):
        pass


class Table:
    """HashTableMatchFinder (hashtable.rs)."""

    def __init__(self):
        self.ht = [0] * CACHE
        self.c = {}

    def get_and_insert(self, data, base, anchor, ip, value):
        min_off = max(base + max(ip - 32768, 0), 1)
        hi = chash(value) % CACHE
        off = self.ht[hi]
        self.ht[hi] = ip + base
        if off >= min_off:
            length, start = match_length(True, value, data, anchor, ip, off - base)
            if length >= 8:
                return [length, ip - (off - base), start]
        return [0, 0, 0]

    def insert(self, value, off):
        self.ht[chash(value) % CACHE] = off


class Chain:
    """HashChainMatchFinder (hashchain.rs:40-114), statement by statement."""

    def __init__(self, min_match, depth, nice):
        self.ht = [0] * CACHE
        self.links = [0] * W
        self.written = bytearray(W)     # instrumentation only
        self.depth, self.nice, self.min_match = depth, nice, min_match
        self.min8 = min_match == 8
        self.mask = M64 >> (8 * (8 - min_match))
        self.c = dict(steps2=0, nice=0, eod=0, alias=0, depth=0, unwritten=0, maxsteps=0)

    def get_and_insert(self, data, base, anchor, ip, value):
        c = self.c
        min_off = max(base + max(ip - 32768, 0), 1)
        best_off, best_len, best_start = 0, self.min_match - 1, 0
        n = self.depth
        hi = chash(value & self.mask) % CACHE
        off = self.ht[hi]
        new = ip + base
        self.ht[hi] = new
        self.links[new % W] = off       # before the walk
        self.written[new % W] = 1
        steps = 0
        while True:
            if off < min_off:
                break
            steps += 1
            if steps >= 2:
                c["steps2"] += 1
            if off == new - 32768:
                c["alias"] += 1
            length, start = match_length(self.min8, value, data, anchor, ip, off - base)
            if length > best_len:
                best_len, best_off, best_start = length, off, start
            if length >= self.nice:
                c["nice"] += 1
                break
            if ip + length == len(data):
                c["eod"] += 1
                break
            n -= 1
            if n == 0:
                c["depth"] += 1
                break
            if not self.written[off % W]:
                c["unwritten"] += 1
            off = self.links[off % W]
        if steps > c["maxsteps"]:
            c["maxsteps"] = steps
        if best_len >= self.min_match:
            return [best_len, ip - (best_off - base), best_start]
        return [0, 0, 0]

    def insert(self, value, off):
        hi = chash(value & self.mask) % CACHE
        prev = self.ht[hi]
        self.ht[hi] = off
        self.links[off % W] = prev
        self.written[off % W] = 1


# ---- bit writer (bitwriter.rs): LSB first ----
class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nbits = 0

    def bits(self, value, n):
        self.acc |= value << self.nbits
        self.nbits += n
        if self.nbits >= 4096:
            k = self.nbits // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.nbits -= 8 * k

    def flush(self):    # pad to a byte
        k = (self.nbits + 7) // 8
        self.out += self.acc.to_bytes(k, "little")
        self.acc = 0
        self.nbits = 0

    def raw(self, b):
        assert self.nbits == 0
        self.out += b


# ---- build_huffman_tree (bitstream.rs:198-325), heap order as oracle/fdeflate_oracle.c restates it ----
# heap items are (frequency, index); Ord is reversed on the frequency alone: a <= b  <=>  a.f >= b.f
def _sift_down_range(d, pos, end):
    elem = d[pos]
    hole, child = pos, 2 * pos + 1
    lim = end - 2 if end >= 2 else 0
    while child <= lim:
        if d[child][0] >= d[child + 1][0]:
            child += 1
        if elem[0] <= d[child][0]:
            d[hole] = elem
            return
        d[hole] = d[child]
        hole = child
        child = 2 * hole + 1
    if child == end - 1 and elem[0] > d[child][0]:
        d[hole] = d[child]
        hole = child
    d[hole] = elem


def _heap_pop(d):
    item = d.pop()
    if d:
        item, d[0] = d[0], item
        end, hole, child = len(d), 0, 1
        elem = d[0]
        lim = end - 2 if end >= 2 else 0
        while child <= lim:
            if d[child][0] >= d[child + 1][0]:
                child += 1
            d[hole] = d[child]
            hole = child
            child = 2 * hole + 1
        if child == end - 1:
            d[hole] = d[child]
            hole = child
        while hole > 0:
            parent = (hole - 1) // 2
            if elem[0] >= d[parent][0]:
                break
            d[hole] = d[parent]
            hole = parent
        d[hole] = elem
    return item


def build_huffman_tree(freq, limit):
    n = len(freq)
    lengths = [0] * n
    codes = [0] * n
    used = [i for i in range(n) if freq[i] > 0]
    if len(used) <= 1:
        if used:
            lengths[used[0]] = 1
        return lengths, codes
    heap = [(freq[i], i) for i in used]
    for k in range(len(heap) // 2 - 1, -1, -1):
        _sift_down_range(heap, k, len(heap))
    left, right = [], []
    while len(heap) > 1:
        a = _heap_pop(heap)
        left.append(a[1])
        right.append(heap[0][1])
        heap[0] = (a[0] + heap[0][0], len(left) + n - 1)
        _sift_down_range(heap, 0, len(heap))
    stack = [(heap[0][1], 0)]
    while stack:
        node, depth = stack.pop()
        if node < n:
            lengths[node] = depth
        else:
            stack.append((left[node - n], depth + 1))
            stack.append((right[node - n], depth + 1))
    if max(lengths) > limit:
        counts = [0] * 16
        for l in lengths:
            counts[min(l, limit)] += 1
        total = sum(counts[i] << (limit - i) for i in range(1, limit + 1))
        while total > (1 << limit):
            i = limit - 1
            while counts[i] == 0:
                i -= 1
            counts[i] -= 1
            counts[limit] -= 1
            counts[i + 1] += 2
            total -= 1
        order = sorted(range(n), key=lambda i: freq[i])     # stable, as the oracle restates it
        ln = limit
        for i in order:
            if freq[i] > 0:
                while counts[ln] == 0:
                    ln -= 1
                lengths[i] = ln
                counts[ln] -= 1
    code = 0
    for ln in range(1, limit + 1):
        for i in range(n):
            if lengths[i] == ln:
                codes[i] = int(format(code, "0%db" % ln)[::-1], 2)
                code += 1
        code <<= 1
    return lengths, codes


def dist_sym_of(distance):
    return bisect.bisect_right(DIST_BASE, distance) - 1


def write_block(w, data, symbols, eof):
    """bitstream.rs:41-195.  data is the whole input, literal runs hold absolute positions."""
    freq = [0] * 286
    dfreq = [0] * 30
    freq[256] = 1
    lit = bytearray()
    for s in symbols:
        if s[0] == "L":
            lit += data[s[1]:s[2]]
        else:
            freq[LENGTH_TO_SYMBOL[s[1] - 3]] += 1
            dfreq[dist_sym_of(s[2])] += 1
    if lit:
        bc = np.bincount(np.frombuffer(bytes(lit), dtype=np.uint8), minlength=256)
        for i in range(256):
            freq[i] += int(bc[i])
    lengths, codes = build_huffman_tree(freq, 15)
    dlengths, dcodes = build_huffman_tree(dfreq, 15)
    nl, nd = 286, 30
    while nl > 257 and lengths[nl - 1] == 0:
        nl -= 1
    while nd > 1 and dlengths[nd - 1] == 0:
        nd -= 1
    clfreq = [0] * 19
    for l in lengths[:nl] + dlengths[:nd]:
        clfreq[l] += 1
    cll, clc = build_huffman_tree(clfreq, 7)
    w.bits(5 if eof else 4, 3)
    w.bits(nl - 257, 5)
    w.bits(nd - 1, 5)
    w.bits(15, 4)
    for j in range(19):
        w.bits(cll[CLCL_ORDER[j]], 3)
    for l in lengths[:nl] + dlengths[:nd]:
        w.bits(clc[l], cll[l])
    bits = w.bits
    for s in symbols:
        if s[0] == "L":
            for b in data[s[1]:s[2]]:
                bits(codes[b], lengths[b])
        else:
            _, length, distance = s
            sym = LENGTH_TO_SYMBOL[length - 3]
            bits(codes[sym], lengths[sym])
            e = LENGTH_TO_EXTRA[length - 3]
            bits((length - 3) & ((1 << e) - 1), e)
            ds = dist_sym_of(distance)
            bits(dcodes[ds], dlengths[ds])
            bits(distance - DIST_BASE[ds], DIST_EXTRA[ds])
    bits(codes[256], lengths[256])


class Parser:
    """ParserInner (parse/mod.rs) with GreedyParser::compress (parse/greedy.rs:27-91) and
    RleParser::compress (parse/rle.rs:22-47).  `whole` is the caller's buffer: symbols hold absolute
    positions (base_index + position in the pass's slice)."""

    def __init__(self, shift, mf, rle, w, whole):
        self.shift, self.mf, self.rle, self.w, self.whole = shift, mf, rle, w, whole
        self.symbols = []
        self.ip = self.last_match = self.last_block_end = 0
        self.last_index = 0
        self.m = [0, 0, 0]

    def get_match(self, data, base, fizzle):
        cur = ld64(data, self.ip)
        if (cur & 0xFFFFFFFF) == ((cur >> 8) & 0xFFFFFFFF):
            m = rle_match(data, self.last_match, self.ip)
            self.ip = m[2] + m[0] - 3
            return m
        anchor = self.ip if fizzle else self.last_match
        m = self.mf.get_and_insert(data, base, anchor, self.ip, cur)
        if fizzle and m[0]:
            start, prev = m[2], m[2] - m[1]
            lim = min(258 - m[0], start - self.last_match, max(prev - 1, 0))
            while (m[0] < 258 and m[2] > self.last_match and m[2] > m[1] + 1
                   and data[m[2] - 1] == data[m[2] - m[1] - 1]):
                m[0] += 1
                m[2] -= 1
            _note_exit("match_back", lim, start - m[2], prev)
        assert m[0] == 0 or self.last_match <= m[2]
        self.ip += 1
        return m

    def advance_to_match(self, data, base, max_ip):
        while self.ip < max_ip:
            m = self.get_match(data, base, False)
            if m[0]:
                return m
            self.ip += (self.ip - self.last_match) >> self.shift
        return [0, 0, 0]

    def advance(self, data, base, end):
        assert self.last_match <= self.ip
        insert = self.mf.insert
        for j in range(self.ip, min(end, len(data) - 8)):
            insert(ld64(data, j), base + j)
        self.ip = max(self.ip, end)

    def insert_match(self, base, m):
        assert self.last_match <= m[2]
        if m[2] > self.last_match:
            self.symbols.append(("L", base + self.last_match, base + m[2]))
        self.symbols.append(("B", m[0], m[1]))
        self.last_match = m[2] + m[0]

    def write_block_if_ready(self, data, finish):
        if len(self.symbols) >= BLOCK_SYMBOLS:
            write_block(self.w, self.whole, self.symbols, finish and self.last_match == len(data))
            self.symbols = []
            self.last_block_end = self.last_match

    def compress(self, data, base, start, finish):
        if finish and len(data) == start:       # compress/mod.rs:234-238
            self.w.bits(3, 10)
            self.w.flush()
            return 0
        delta = base - self.last_index          # start_compress
        self.ip -= delta
        self.last_match -= delta
        self.last_block_end = start
        self.last_index = base
        if self.rle:
            lookahead = 7 if finish else 258
            max_ip = max(len(data) - lookahead, 0)
            while True:
                m = self.advance_to_match(data, base, max_ip)
                if not m[0]:
                    break
                self.ip = m[2] + m[0]
                self.insert_match(base, m)
                self.write_block_if_ready(data, finish)
        else:
            if self.m[0]:
                self.m[2] -= delta
            lookahead = 7 if finish else 258 + 8
            max_ip = max(len(data) - lookahead, 0)
            while True:
                if not self.m[0]:
                    self.m = self.advance_to_match(data, base, max_ip)
                    if not self.m[0]:
                        break
                self.advance(data, base, self.m[2] + self.m[0])
                m2 = [0, 0, 0]
                if self.ip < max_ip:
                    m2 = self.get_match(data, base, True)
                elif not finish:
                    break
                if not m2[0] or m2[2] > self.m[2] + 1:
                    self.insert_match(base, self.m)
                    self.write_block_if_ready(data, finish)
                    if m2[0] and m2[2] < self.last_match:
                        assert m2[0] >= 3
                        m2[0] -= self.last_match - m2[2]
                        m2[2] = self.last_match
                        if m2[0] < 4:
                            m2 = [0, 0, 0]
                self.m = m2
        if finish and (self.symbols or self.last_match < len(data)):    # end_compress
            self.ip = min(self.ip, len(data))
            if self.last_match < len(data):
                self.symbols.append(("L", base + self.last_match, base + len(data)))
                self.ip = self.last_match = len(data)
            write_block(self.w, self.whole, self.symbols, True)
            self.symbols = []
            self.last_block_end = self.ip
        return self.last_block_end - start


def _compress(data, shift, mf, rle):
    global last_counters, last_exits
    _exits.clear()
    data = bytes(data)
    assert len(data) <= 1 << 30
    w = BitWriter()
    w.raw(b"\x78\x01")
    p = Parser(shift, mf, rle, w, data)
    window = 1 if rle else W
    written = p.compress(data, 0, 0, False)                 # Compressor::write_data, nothing buffered
    start = max(written - window, 0)
    p.compress(data[start:], start, written - start, True)  # Compressor::finish over the kept tail
    w.flush()
    w.raw((zlib.adler32(data) & 0xFFFFFFFF).to_bytes(4, "big"))
    last_counters = dict(mf.c)
    last_exits = collections.Counter(_exits)
    return bytes(w.out)


def compress(data, level):
    """compress_to_vec_with_level(data, level) for level 1, 2 or 3 (compress/mod.rs:76-79)."""
    if level == 1:
        return _compress(data, 5, Table(), False)
    if level == 2:
        return _compress(data, 6, Chain(8, 16, 64), False)
    if level == 3:
        return _compress(data, 6, Chain(6, 16, 32), False)
    raise ValueError("level %r is not modelled" % (level,))


def compress_rle(data):
    """compress_to_vec_rle(data) (compress/mod.rs:107-123, :306-310)."""
    return _compress(data, 5, Null(), True)


@functools.lru_cache(maxsize=None)
def model_results():
    """level -> (list of (input, stream, counters)) over the encoder inputs, the chain inputs and the run-edge inputs
    of tests/streams.py, and "exits" -> the sum of last_exits over all of them; computed once per process (the GPU
    tests use the same streams as expected bytes)."""
    import streams
    inputs = streams.encoder_inputs() + streams.chain_inputs() + streams.run_edge_inputs()
    res = {"exits": collections.Counter()}
    for level in (2, 3):
        rows = []
        for x in inputs:
            out = compress(x, level)
            rows.append((x, out, dict(last_counters)))
            res["exits"] += last_exits
        res[level] = rows
    return res


@functools.lru_cache(maxsize=None)
def oracle_level_results():
    """Level 1 and RLE, which the oracle has too, over the encoder inputs and the run-edge inputs: "inputs", 1 and
    "rle" -> the model's streams in that order, "exits" -> the sum of last_exits; computed once per process."""
    import streams
    res = {"inputs": streams.encoder_inputs() + streams.run_edge_inputs(), 1: [], "rle": [], "exits": collections.Counter()}
    for x in res["inputs"]:
        res[1].append(compress(x, 1))
        res["exits"] += last_exits
        res["rle"].append(compress_rle(x))
        res["exits"] += last_exits
    return res
