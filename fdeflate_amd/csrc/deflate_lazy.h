// deflate_lazy.h -- the parser kernel of encoder levels 4-9 (include/fdeflate_hip_levels.h): LazyParser
// (src/compress/parse/lazy.rs:31-117) over HybridMatchFinder (src/compress/matchfinder/hybrid.rs:40-162), one stream per
// lane, bit-exact with the reference.  Included by deflate_general.hip behind GParserT, whose pieces of ParserInner it
// uses as they are (the counters of equal bytes, match_length::<false>, rle_match, insert_match, write_block_if_ready,
// start_compress, end_compress); it records GMatchRec / GBlockRec like deflate_parse_kernel and the block writer does
// not know which of the two ran.  A kernel of its own, so that the parsers of levels 1-3 stay the code they were.
//
// The level's five parameters (launch.h, LazyParams) are kernel arguments, uniform over the launch: one instance of the
// code instead of four, and nothing the parameters select is worth a register -- the time goes into dependent loads.
//
// Tables, per resident stream 640 KiB: the head table (hashed on min_match + 1 bytes, `mask`), the 4-table (hashed on
// min_match bytes, `mask4`) and the ring of 32 768 links.  Both tables start as zeros for every stream
// (hybrid.rs:28-29) and are cleared by the whole wavefront.  The ring is NOT cleared, by the argument above
// chain_get_and_insert: a link slot is read only for an offset that came out of the head table or out of a link, is
// >= min_offset >= 1, and was therefore stored by lookup / insert of THIS stream, which wrote links[offset % 32768] in
// the same step.  offset4, the 4-table's value, only ever names a position in the data: it never indexes the ring.
// (tests/lazy_model.py counts reads of slots the stream has not written and finds none.)
#pragma once

namespace fdh {

struct GLazyParser : GParserT<0> {
    uint32_t* hash4;  // this lane's 4-table (`hash` is the head table, `links` the ring, `m` is m1)
    GMatch m0;        // the match m1 displaced, deferred until it is known how much of it survives
    LazyParams P;
    uint64_t mask, mask4;  // hybrid.rs:35-36

    // "Visit previous matches" and the rescue through the 4-table (hybrid.rs:75-126) for the position at `ip`, which
    // is in all three tables already.  offset / offset4: what the head table / the 4-table held before.  As written
    // there: the walk breaks on offset < min_offset, the rescue wants offset4 > min_offset; it happens only while
    // best_length < the FINDER's min_match and overwrites best_length with whatever match_length gives, 0 included;
    // the depth is a quarter when the call asks for more than the finder's min_match (every lazy probe does);
    // `l > best_length` is strict; `ip + l == len` takes the caller's ip and the pass's slice.
    __device__ GMatch walk(const uint8_t* data, uint64_t len, uint32_t base_index, uint64_t anchor, uint64_t value, uint32_t offset,
                           uint32_t offset4, uint32_t min_match) {
        const uint32_t oldest = min_offset(base_index, ip);
        uint32_t best_offset = 0, best_length = min_match - 1;
        uint64_t best_start = 0;
        uint32_t l;
        uint64_t st;
#pragma nounroll
        for (uint32_t n = min_match > P.min_match ? P.depth >> 2 : P.depth; offset >= oldest;) {
            const uint32_t next = links[offset % kGWindow];  // fetched with the candidate's bytes (see chain_walk)
            match_length<false>(value, data, len, anchor, ip, (uint64_t)(offset - base_index), l, st);
            if (l > best_length) {
                best_length = l;
                best_offset = offset;
                best_start = st;
            }
            if (l >= P.nice || ip + l == len) break;
            if (--n == 0) break;
            offset = next;
        }
        if (best_length < P.min_match && offset4 > oldest) {
            match_length<false>(value, data, len, anchor, ip, (uint64_t)(offset4 - base_index), l, st);
            best_length = l;
            best_offset = offset4;
            best_start = st;
        }
        if (best_length >= min_match) return GMatch{best_length, (uint32_t)(ip - (uint64_t)(best_offset - base_index)), best_start};
        return GMatch{0, 0, 0};
    }

    // get_and_insert_lazy (hybrid.rs:129-139) at ip: the new position goes into the head table, the ring AND the
    // 4-table before the walk, so a candidate at exactly ip - 32768 reads the slot just replaced, as in the chain finder
    __device__ GMatch lazy_probe(const uint8_t* data, uint64_t len, uint32_t base_index, uint32_t min_match) {
        const uint64_t value = g_load64(data + ip);
        const uint32_t h = g_hash(value & mask), h4 = g_hash(value & mask4);
        const uint32_t offset = hash[h], offset4 = hash4[h4];
        const uint32_t new_offset = (uint32_t)ip + base_index;
        hash[h] = new_offset;
        links[new_offset % kGWindow] = offset;
        hash4[h4] = new_offset;
        return walk(data, len, base_index, last_match, value, offset, offset4, min_match);
    }

    // ParserInner::advance_to_match (parse/mod.rs:88-102) with get_match(fizzle = false) and lookup(.., min_match 4):
    // GParserT::advance_to_match's grouped look-ahead -- the loads of kGroup steps in flight while nothing is found, the
    // decisions in order, table values that an earlier step of the group replaced patched from registers -- with two
    // table loads per step.  A step has a candidate when the head's old value is >= min_offset or the 4-table's is
    // > min_offset; its walk runs behind the unrolled part.  Half the chain parsers' group: a step holds two hashes and
    // two table values.
    static constexpr int kGroup = 8;
    __device__ GMatch advance_to_match(const uint8_t* data, uint64_t len, uint32_t base_index, uint64_t max_ip) {
        while (ip < max_ip) {
            uint64_t p[kGroup], cur[kGroup];
            uint32_t h[kGroup], h4[kGroup], off[kGroup], off4[kGroup];
            uint64_t q = ip;
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                p[k] = q;
                cur[k] = g_load64(data + (q < max_ip ? q : ip));
                q++;
                q += (q - last_match) >> P.shift;
            }
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                h[k] = g_hash(cur[k] & mask);
                h4[k] = g_hash(cur[k] & mask4);
                off[k] = hash[h[k]];
                off4[k] = hash4[h4[k]];
            }
            int event = 0;  // 1 end of the scan range, 2 a run (RLE pattern), 3 a candidate from either table
            uint64_t ev_p = 0, ev_cur = 0;
            uint32_t ev_off = 0, ev_off4 = 0;
#pragma unroll
            for (int k = 0; k < kGroup; k++) {
                if (event == 0) {
                    ev_p = p[k];
                    ev_cur = cur[k];
                    if (p[k] >= max_ip) {
                        event = 1;
                    } else if ((uint32_t)cur[k] == (uint32_t)(cur[k] >> 8)) {
                        event = 2;
                    } else {  // the insert of lookup (hybrid.rs:60-73)
                        uint32_t offset = off[k], offset4 = off4[k];
#pragma unroll
                        for (int j = 0; j < k; j++) {
                            if (h[j] == h[k]) offset = (uint32_t)p[j] + base_index;
                            if (h4[j] == h4[k]) offset4 = (uint32_t)p[j] + base_index;
                        }
                        const uint32_t new_offset = (uint32_t)p[k] + base_index;
                        hash[h[k]] = new_offset;
                        links[new_offset % kGWindow] = offset;
                        hash4[h4[k]] = new_offset;
                        const uint32_t oldest = min_offset(base_index, p[k]);
                        if (offset >= oldest || offset4 > oldest) {
                            event = 3;
                            ev_off = offset;
                            ev_off4 = offset4;
                        }
                    }
                }
            }
            if (event == 0) {
                ip = q;
                continue;
            }
            ip = ev_p;
            if (event == 1) return GMatch{0, 0, 0};
            if (event == 2) {  // ParserInner::get_match (parse/mod.rs:60-63)
                const GMatch r = rle_match(data, len);
                ip = r.end() - 3;
                return r;
            }
            const GMatch r = walk(data, len, base_index, last_match, ev_cur, ev_off, ev_off4, 4);
            ip++;
            if (r.length != 0) return r;
            ip += (ip - last_match) >> P.shift;
        }
        return GMatch{0, 0, 0};
    }

    // ParserInner::advance (parse/mod.rs:105-114) with HybridMatchFinder::insert (hybrid.rs:154-162): the data of four
    // positions is fetched together, the tables are updated in position order
    __device__ void insert(uint64_t value, uint32_t offset) {
        hash4[g_hash(value & mask4)] = offset;
        const uint32_t h = g_hash(value & mask);
        const uint32_t prev = hash[h];
        hash[h] = offset;
        links[offset % kGWindow] = prev;
    }
    __device__ void advance(const uint8_t* data, uint64_t len, uint32_t base_index, uint64_t end) {
        const uint64_t stop = min(end, len - 8);
        uint64_t j = ip;
        for (; j + 4 <= stop; j += 4) {
            const uint64_t v0 = g_load64(data + j), v1 = g_load64(data + j + 1), v2 = g_load64(data + j + 2), v3 = g_load64(data + j + 3);
            insert(v0, base_index + (uint32_t)j);
            insert(v1, base_index + (uint32_t)j + 1);
            insert(v2, base_index + (uint32_t)j + 2);
            insert(v3, base_index + (uint32_t)j + 3);
        }
        for (; j < stop; j++) insert(g_load64(data + j), base_index + (uint32_t)j);
        ip = max(ip, end);
    }

    // CompressorInner::compress (compress/mod.rs:226-290) -> LazyParser::compress (lazy.rs:31-117).  m0 and m1 survive
    // between the two passes of a stream: a Flush::None pass leaves the loop with m1 found and not emitted, and the
    // finishing pass resumes it without searching again.  write_block_if_ready is reached only where a later-starting
    // m2 displaces m1 (the other branches `continue`), so a block can hold more than 16 384 symbols: g_block_slice's
    // bound only gets looser.  Every back-reference recorded is still at least 4 bytes long and none overlap -- m1
    // comes from rle_match (>= 4) or from lookup with min_match >= 4, anchored at last_match; the deferred m0 goes out
    // only when it starts 4 bytes or more in front of m1, cut to end where m1 starts -- so g_match_slice's len / 4 holds.
    __device__ uint64_t compress(const uint8_t* data, uint64_t len, uint32_t base_index, uint64_t start, bool finish) {
        if (finish && len == start) {  // :234-238
            record_block(base_index + (uint32_t)len, kGBlockEmptyFixed);
            return 0;
        }
        const uint64_t delta = start_compress(base_index, start);
        if (m0.length != 0) m0.start -= delta;
        if (m.length != 0) m.start -= delta;
        const uint64_t lookahead = finish ? 7 : 258 + 8;
        const uint64_t max_ip = len > lookahead ? len - lookahead : 0;
        for (;;) {
            if (m.length == 0) {
                m = advance_to_match(data, len, base_index, max_ip);
                if (m.length == 0) break;
            }
            GMatch m2{0, 0, 0};
            if (m.length <= P.max_lazy) {
                if (ip < max_ip) {  // (only then are there 8 bytes to read at ip)
                    m2 = lazy_probe(data, len, base_index, m.length + 1);
                    ip++;
                    if (m2.length <= m.length) m2 = GMatch{0, 0, 0};
                } else if (!finish) {
                    break;
                }
            }
            if (m2.length == 0) {
                advance(data, len, base_index, m.end());
                if (m0.length != 0 && m0.start + 4 <= m.start) {
                    m0.length = min(m0.length, (uint32_t)(m.start - m0.start));
                    insert_match(base_index, m0);
                }
                insert_match(base_index, m);
                m0 = GMatch{0, 0, 0};
                m = GMatch{0, 0, 0};
                continue;
            }
            if (m2.start <= m.start) {
                m = m2;
                continue;
            }
            if (m0.length == 0 || m.start < m0.start || (m.start == m0.start && m.length > m0.length)) m0 = m;
            m = m2;
            write_block_if_ready(len, base_index, finish);
        }
        return end_compress(len, base_index, start, finish);
    }
};

// deflate_parse_kernel's frame for the lazy levels.  a.hash: per wavefront the L head tables and the L 4-tables (cleared
// together for every round of streams), then the L link rings (not cleared: above).
__global__ __launch_bounds__(kWave) void deflate_lazy_parse_kernel(GParseArgs a, LazyParams P) {
    const uint32_t lane = threadIdx.x;
    const uint32_t L = a.lanes;
    const uint64_t in0 = a.in_off[0];
    uint32_t* wave_hash = a.hash + (uint64_t)blockIdx.x * L * (2 * kGHashSize + kGWindow);
    for (uint64_t sid0 = (uint64_t)blockIdx.x * L; sid0 < a.n; sid0 += (uint64_t)gridDim.x * L) {
        uint4* t = reinterpret_cast<uint4*>(wave_hash);
        for (uint32_t i = lane; i < 2 * L * (kGHashSize / 4); i += kWave) t[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint64_t sid = sid0 + lane;
        if (lane >= L || sid >= a.n) continue;
        const uint64_t off = a.in_off[sid];
        const uint8_t* input = a.in + off;
        const uint64_t len = a.in_off[sid + 1] - off;
        if (len > (1ull << 30)) {  // write_data splits above 1 GiB (compress/mod.rs:130-136): not supported
            a.nblocks[sid] = 0xFFFFFFFFu;
            continue;
        }
        GLazyParser ps;
        ps.hash = wave_hash + (uint64_t)lane * kGHashSize;
        ps.hash4 = wave_hash + ((uint64_t)L + lane) * kGHashSize;
        ps.links = wave_hash + 2 * (uint64_t)L * kGHashSize + (uint64_t)lane * kGWindow;
        ps.mrec = a.matches + g_match_slice(off - in0, sid);
        ps.brec = a.blocks + g_block_slice(off - in0, sid);
        ps.nmatch = ps.nblock = ps.nsym = 0;
        ps.ip = ps.last_match = ps.last_block_end = 0;
        ps.last_index = 0;
        ps.m = ps.m0 = GMatch{0, 0, 0};
        ps.P = P;
        ps.mask = ~0ull >> (8 * (8 - (P.min_match + 1)));  // min_match is 4 or 5: (min_match + 1).min(8) is min_match + 1
        ps.mask4 = ~0ull >> (8 * (8 - P.min_match));
#ifdef FDH_DEBUG_GEN
        for (int k = 0; k < 8; k++) ps.tacc[k] = 0;
#endif
        // Compressor::write_data with Flush::None, then Compressor::finish over the kept tail data[start..], as in
        // deflate_parse_kernel: the window is 32 768
        uint64_t written = 0, start = 0;
#pragma nounroll
        for (int pass = 0; pass < 2; pass++) {
            if (pass) start = written > kGWindow ? written - kGWindow : 0;
            const uint64_t r = ps.compress(input + start, len - start, (uint32_t)start, pass ? written - start : 0, pass != 0);
            if (!pass) written = r;
        }
        a.nblocks[sid] = ps.nblock;
    }
}

}  // namespace fdh
