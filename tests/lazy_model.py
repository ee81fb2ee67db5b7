"""Pure-Python restatement of the reference's encoder at levels 4-9: LazyParser (src/compress/parse/lazy.rs:31-117)
over HybridMatchFinder (src/compress/matchfinder/hybrid.rs:40-162), whole zlib streams, no compiled code.

Everything the lazy levels share with levels 1-3 is tests/level_model.py's and is imported from there: ParserInner's
pieces (`Parser.get_match`, `advance_to_match`, `advance`, `insert_match`, `write_block_if_ready`), `match_length`,
`rle_match`, `write_block`, `BitWriter` and the two-pass driver `_compress` -- all pinned against the oracle at level 1
and RLE by tests/test_level_model.py.  What is stated here is `Hybrid` and `LazyParser.compress`, about 150 lines.  The
oracle restates the same two pieces in C from the Rust (fdo_compress_level, levels 4..9), written apart from this
file: two readings, which tests/test_oracle_levels.py holds to the same bytes and, counter by counter, to the same
branch counts over shared_inputs().  A misreading both share stays possible: there is no Rust toolchain to run the crate.

`compress(data, level)` serves levels 4..9 (7, 8 and 9 are one parameter set, compress/mod.rs:80-87).  The counters of
the last call are in `last_counters`:
  finder   steps2, nice, eod, depth, alias, unwritten, maxsteps   as level_model.Chain counts them
           quarter        lookups whose depth was cut to search_depth >> 2 (the call's min_match above the finder's)
           rescue_hit     the 4-table's candidate replaced the walk's result and gave a match
           rescue_miss    ... and left fewer bytes than the call asked for: the empty match
           rescue_zero    ... and match_length returned 0 (a subset of rescue_miss)
  loop     m0_empty, m0_earlier, m0_longer   the clause by which m1 became the deferred m0; m0_kept: none held
           m0_inserted    the deferred match went out, m0_cut of them shortened to m1.start - m0.start
           m0_dropped     the deferred match began fewer than 4 bytes in front of m1
           m2_same_start  a lazy match that begins at or before m1 replaced it
           pending        a Flush::None pass ended with m1 found and not yet emitted
           resumed        a pass began with the m1 of the pass before
           blocks         write_block_if_ready wrote a block, max_block_symbols: the most symbols it found
           pass2_base     base_index of the second pass
"""
import functools

import level_model as lm
from level_model import CACHE, M64, W, chash, ld64, match_length

# level -> (skip_ahead_shift, max_lazy, (min_match, search_depth, nice_length))   compress/mod.rs:80-87
PARAMS = {4: (9, 12, (5, 16, 32)), 5: (9, 16, (5, 64, 64)), 6: (9, 16, (4, 128, 128)), 7: (12, 256, (4, 256, 258))}
PARAMS[8] = PARAMS[9] = PARAMS[7]

FINDER_COUNTERS = ("steps2", "nice", "eod", "depth", "alias", "unwritten", "maxsteps", "quarter", "rescue_hit", "rescue_miss",
                   "rescue_zero")
LOOP_COUNTERS = ("m0_empty", "m0_earlier", "m0_longer", "m0_kept", "m0_inserted", "m0_cut", "m0_dropped", "m2_same_start",
                 "pending", "resumed", "blocks", "max_block_symbols", "pass2_base")
MAX_COUNTERS = ("maxsteps", "max_block_symbols", "pass2_base")     # summed over inputs by max, the others by +

last_counters = {}


class Hybrid:
    """HybridMatchFinder (hybrid.rs:40-162), statement by statement."""

    def __init__(self, min_match, depth, nice):
        assert 4 <= min_match <= 7
        self.ht = [0] * CACHE
        self.ht4 = [0] * CACHE
        self.links = [0] * W
        self.written = bytearray(W)     # instrumentation only
        self.depth, self.nice, self.min_match = depth, nice, min_match
        self.mask = M64 >> (8 * (8 - min(min_match + 1, 8)))
        self.mask4 = M64 >> (8 * (8 - min_match))
        self.c = dict.fromkeys(FINDER_COUNTERS + LOOP_COUNTERS, 0)

    def lookup(self, data, base, anchor, ip, value, min_match):
        c = self.c
        min_off = max(base + max(ip - 32768, 0), 1)
        best_off, best_len, best_start = 0, min_match - 1, 0
        n = self.depth
        if min_match > self.min_match:
            n >>= 2
            c["quarter"] += 1
        hi4 = chash(value & self.mask4) % CACHE
        off4 = self.ht4[hi4]
        hi = chash(value & self.mask) % CACHE
        off = self.ht[hi]
        new = ip + base
        self.ht[hi] = new
        self.links[new % W] = off       # before the walk
        self.written[new % W] = 1
        self.ht4[hi4] = new
        steps = 0
        while True:
            if off < min_off:
                break
            steps += 1
            if steps >= 2:
                c["steps2"] += 1
            if off == new - 32768:
                c["alias"] += 1
            length, start = match_length(False, value, data, anchor, ip, off - base)
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
        if best_len < self.min_match and off4 > min_off:    # `<` walk above, `>` here: as written there
            best_len, best_start = match_length(False, value, data, anchor, ip, off4 - base)
            best_off = off4
            c["rescue_hit" if best_len >= min_match else "rescue_miss"] += 1
            if best_len == 0:
                c["rescue_zero"] += 1
        if best_len >= min_match:
            return [best_len, ip - (best_off - base), best_start]
        return [0, 0, 0]

    def get_and_insert(self, data, base, anchor, ip, value):
        return self.lookup(data, base, anchor, ip, value, 4)

    def get_and_insert_lazy(self, data, base, anchor, ip, value, min_match):
        return self.lookup(data, base, anchor, ip, value, min_match)

    def insert(self, value, off):
        self.ht4[chash(value & self.mask4) % CACHE] = off
        hi = chash(value & self.mask) % CACHE
        prev = self.ht[hi]
        self.ht[hi] = off
        self.links[off % W] = prev
        self.written[off % W] = 1


class LazyParser(lm.Parser):
    """ParserInner as level_model.Parser has it, with LazyParser::compress (lazy.rs:31-117) in place of the greedy loop.
    Built by level_model._compress, so with Parser's arguments: max_lazy rides on the finder."""

    def __init__(self, shift, mf, rle, w, whole):
        assert not rle
        super().__init__(shift, mf, rle, w, whole)
        self.max_lazy = mf.max_lazy
        self.m0 = [0, 0, 0]
        self.m1 = [0, 0, 0]

    def compress(self, data, base, start, finish):
        c = self.mf.c
        if finish and len(data) == start:       # compress/mod.rs:234-238
            self.w.bits(3, 10)
            self.w.flush()
            return 0
        delta = base - self.last_index          # start_compress
        self.ip -= delta
        self.last_match -= delta
        self.last_block_end = start
        self.last_index = base
        if self.m0[0]:
            self.m0[2] -= delta
        if self.m1[0]:
            self.m1[2] -= delta
            c["resumed"] += 1
        if finish:
            c["pass2_base"] = base
        lookahead = 7 if finish else 258 + 8
        max_ip = max(len(data) - lookahead, 0)
        while True:
            if not self.m1[0]:
                self.m1 = self.advance_to_match(data, base, max_ip)
                if not self.m1[0]:
                    break
            m0, m1 = self.m0, self.m1
            assert self.last_match <= self.ip and self.last_match <= m1[2]
            m2 = [0, 0, 0]
            if m1[0] <= self.max_lazy:
                if self.ip < max_ip:
                    assert self.ip < m1[2] + m1[0]
                    m2 = self.mf.get_and_insert_lazy(data, base, self.last_match, self.ip, ld64(data, self.ip), m1[0] + 1)
                    self.ip += 1
                    if m2[0] <= m1[0]:
                        m2 = [0, 0, 0]
                elif not finish:
                    c["pending"] += 1
                    break
            if not m2[0]:
                self.advance(data, base, m1[2] + m1[0])
                if m0[0] and m0[2] + 4 <= m1[2]:
                    c["m0_inserted"] += 1
                    if m1[2] - m0[2] < m0[0]:
                        c["m0_cut"] += 1
                        m0[0] = m1[2] - m0[2]
                    self.insert_match(base, m0)
                elif m0[0]:
                    c["m0_dropped"] += 1
                self.insert_match(base, m1)
                self.m0 = [0, 0, 0]
                self.m1 = [0, 0, 0]
                continue
            elif m2[2] <= m1[2]:
                c["m2_same_start"] += 1
                self.m1 = m2
                continue
            else:
                assert m1[0] < m2[0]
                if not m0[0]:
                    c["m0_empty"] += 1
                    self.m0 = m1
                elif m1[2] < m0[2]:
                    c["m0_earlier"] += 1
                    self.m0 = m1
                elif m1[2] == m0[2] and m1[0] > m0[0]:
                    c["m0_longer"] += 1
                    self.m0 = m1
                else:
                    c["m0_kept"] += 1
                self.m1 = m2
            if len(self.symbols) >= lm.BLOCK_SYMBOLS:   # the only place a block is cut: it can hold more than 16 384 symbols
                c["blocks"] += 1
                c["max_block_symbols"] = max(c["max_block_symbols"], len(self.symbols))
            self.write_block_if_ready(data, finish)
        if finish and (self.symbols or self.last_match < len(data)):    # end_compress
            self.ip = min(self.ip, len(data))
            if self.last_match < len(data):
                self.symbols.append(("L", base + self.last_match, base + len(data)))
                self.ip = self.last_match = len(data)
            lm.write_block(self.w, self.whole, self.symbols, True)
            self.symbols = []
            self.last_block_end = self.ip
        return self.last_block_end - start


def compress(data, level):
    """compress_to_vec_with_level(data, level) for level 4..9 (compress/mod.rs:80-87)."""
    global last_counters
    if isinstance(level, bool) or not isinstance(level, int) or level not in PARAMS:
        raise ValueError("level %r is not modelled here" % (level,))
    shift, max_lazy, finder = PARAMS[level]
    mf = Hybrid(*finder)
    mf.max_lazy = max_lazy
    # level_model._compress builds its parser as `Parser(shift, mf, rle, w, data)`: for the duration of the call that name
    # is the lazy parser, so that the two passes, the window and the trailer are the driver the oracle pins
    greedy = lm.Parser
    lm.Parser = LazyParser
    try:
        out = lm._compress(data, shift, mf, False)
    finally:
        lm.Parser = greedy
    last_counters = dict(mf.c)
    return out


def add_counters(total, c):
    for k, v in c.items():
        total[k] = max(total.get(k, 0), v) if k in MAX_COUNTERS else total.get(k, 0) + v
    return total


# ---- inputs of the lazy levels' own ----

def short_chain_input(words=9200, seed=41):
    """Every chain is short: each 5-byte word of random bytes occurs exactly twice, a fresh literal behind every word, the
    two occurrences a few hundred words apart: a back-reference and a literal per 12 bytes, so the 16 384th symbol
    comes near 103 000 of the 115 000 bytes, before len - 266.  A block is cut only where a later match displaces m1, so every 40th
    word is a triple instead -- X[0:7], then X[1:12], then X[0:12] for 12 random bytes X: at the third, the match with
    the first (7 bytes) is displaced by the match with the second one byte later (11 bytes).  The first pass therefore
    writes a block, the second starts past 0, and there are deferrals past position 32 768, all without long walks."""
    import numpy as np
    r = np.random.default_rng(seed)
    units = []      # (key, bytes): sorted by key, a literal appended to each
    for i in range(words):
        if i % 40 == 39:
            x = bytes(r.integers(0, 256, 12, dtype=np.uint8))
            units += [(2.0 * i, x[:7]), (2.0 * i + 50, x[1:]), (2.0 * i + 100, x)]
        else:
            w = bytes(r.integers(0, 256, 5, dtype=np.uint8))
            units += [(2.0 * i, w), (2.0 * i + 1 + 600 * float(r.random()), w)]
    units.sort(key=lambda u: u[0])
    lit = r.integers(0, 256, len(units), dtype=np.uint8)
    return b"".join(u + bytes([int(b)]) for (_, u), b in zip(units, lit))


def clause_inputs():
    """Eight inputs of 2 400 .. 4 900 bytes found by a search over seeds: m1 replaces the deferred m0 because it starts
    earlier (seeds 316, 376, 1103, 1262) or starts at the same place and is longer (92, 144, 176, 892), each clause at
    each of the levels 4, 5, 6 and 9 at least once.  Both need a lazy match that reaches backwards past the start of
    m1 while a match is deferred, which noise over two or three symbols gives now and then."""
    import numpy as np
    out = []
    for seed in (92, 144, 176, 316, 376, 892, 1103, 1262):
        r = np.random.default_rng(1000 + seed)
        n = int(r.integers(1500, 5000))
        if seed % 4 == 0:
            x = bytes(r.integers(0, 2, n, dtype=np.uint8) + 65)
        elif seed % 4 == 2:
            ws = [bytes(r.integers(65, 68, int(r.integers(2, 7)), dtype=np.uint8)) for _ in range(8)]
            x = b"".join(ws[int(k)] for k in r.integers(0, 8, n // 4))
        else:
            ws = [bytes(r.integers(65, 69, int(r.integers(3, 9)), dtype=np.uint8)) for _ in range(6)] + [b"AAAAAA", b"BBBBBBB"]
            x = b"".join(ws[int(k)] for k in r.integers(0, 8, n // 5))
        out.append(x)
    return out


def lazy_inputs():
    """Inputs made for the lazy loop and the hybrid finder (seeds fixed):
    [0] short_chain_input();
    [1] overlapping phrases: text over 12 'words' of 3..9 bytes with a shared prefix, so that a match that starts one
        byte later is often longer (deferrals, m0 replaced by every clause, m0 cut and dropped);
    [2] the same kind, 40 000 bytes of an alphabet of 4 (long chains at moderate size: depth exits, quarter depth);
    [3] a phrase repeated to the very end of the buffer (end-of-data exit in a lazy probe);
    [4] 5-byte words whose first four bytes recur with another fifth byte (the 4-table's rescue, hit and miss);
    [5..12] clause_inputs()."""
    import numpy as np
    r = np.random.default_rng(43)
    out = [short_chain_input()]
    stem = bytes(r.integers(97, 123, 4, dtype=np.uint8))
    words = [stem[:int(r.integers(1, 5))] + bytes(r.integers(97, 123, int(r.integers(2, 6)), dtype=np.uint8)) for _ in range(12)]
    out.append(b"".join(words[int(k)] for k in r.integers(0, 12, 6000)))
    out.append(bytes(r.integers(0, 4, 40000, dtype=np.uint8)))
    phrase = bytes(r.integers(0, 256, 40, dtype=np.uint8))
    out.append(bytes(r.integers(0, 256, 300, dtype=np.uint8)) + phrase + b"xyz" + phrase[1:] + b"q" + phrase)
    bb = bytearray()
    heads = [bytes(r.integers(0, 256, 4, dtype=np.uint8)) for _ in range(40)]
    for _ in range(3000):
        bb += heads[int(r.integers(0, 40))] + bytes(r.integers(0, 256, int(r.integers(1, 4)), dtype=np.uint8))
    out.append(bytes(bb))
    return out + clause_inputs()


@functools.lru_cache(maxsize=None)
def shared_inputs():
    """level -> the inputs the CPU and the GPU tests share at that level.  Level 4 (depth 16, as levels 2 and 3): the
    encoder inputs, the chain inputs, the run-edge inputs (which end with the late-match family) and lazy_inputs().
    Levels 5, 6 and 9 (= 7 = 8) walk up to 64, 128 and 256 candidates per position, in Python here and as dependent
    steps of one lane on the device: of the nine long low-entropy inputs (120 000 and 300 000 bytes over an alphabet of
    3 or 4; 110 s of model time at level 6 with all of them, 30 s with one) they keep one, the first 300 000-byte one
    over an alphabet of 4 -- the second pass past 0, two blocks cut and the alias at distance 32 768 are all in it."""
    import streams
    enc, chain = streams.encoder_inputs(), streams.chain_inputs()
    full = enc + chain + streams.run_edge_inputs() + lazy_inputs()
    low = set(chain[:8]) | {x for x in enc if len(x) == 300000}
    keep = chain[3]
    assert len(keep) == 300000 and max(keep) == 3
    lean = [x for x in full if x not in low or x is keep]
    return {4: full, 5: lean, 6: lean, 9: lean}


@functools.lru_cache(maxsize=None)
def model_results():
    """level (4, 5, 6, 9) -> list of (input, stream, counters) over shared_inputs()[level]; computed once per process
    (the GPU tests use the same streams as expected bytes)."""
    res = {}
    for level, inputs in shared_inputs().items():
        rows = []
        for x in inputs:
            out = compress(x, level)
            rows.append((x, out, dict(last_counters)))
        res[level] = rows
    return res
