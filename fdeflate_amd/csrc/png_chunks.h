// png_chunks.h -- the IDAT gather and the PLTE / tRNS reader of png_file.hip as device functions of one file, so that
// png_file.hip (one geometry per call) and png_mixed.hip (the geometry of each file in its fdh_png_info record) run the
// same code behind their own checks.  Not the scan: that stays in png_file.hip.
#pragma once
#include "device_common.h"
#include "png_common.h"
#include "png_record.h"

namespace fdh {

__device__ __forceinline__ uint32_t get_be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

constexpr uint32_t kIHDR = 0x49484452u, kPLTE = 0x504C5445u, kIDAT = 0x49444154u, kIEND = 0x49454E44u;

// ---- fdh_png_gather_idat_batch ----
struct GatherArgs {
    const uint8_t* file;
    const uint64_t* file_off;
    const PngInfo* info;
    uint8_t* comp;
    const uint64_t* comp_off;
    uint32_t* comp_len;
    uint32_t* png_status;
    uint64_t n;
    uint32_t width, bit_depth, colour_type;
};

struct __attribute__((packed, aligned(1))) Bytes16 {
    uint32_t x, y, z, w;
};

// One file per workgroup: the IDAT bodies one behind the other.  A body is copied by all lanes: the bytes up to the
// destination's next 16-byte boundary one per lane, then 16 per lane and step (aligned stores; the loads are as aligned as
// the file happens to be), then the rest one per lane.  Reads stay inside the file's slot, writes inside idat_bytes.
// `r` is the file's record; `st` what the caller's checks of it and of the comp slot found (kPngOk: copy).
template <int THREADS>
__device__ __forceinline__ void png_gather_file(const GatherArgs& a, uint64_t i, const PngInfo& r, uint32_t st) {
    const uint64_t o = a.file_off[i], slot = a.file_off[i + 1] - o;
    const uint64_t co = a.comp_off[i];
    if (st) {
        if (threadIdx.x == 0) {
            a.png_status[i] = st;
            a.comp_len[i] = 0;
        }
        return;
    }
    const uint8_t* f = a.file + o;
    uint8_t* dst = a.comp + co;
    uint64_t pos = r.first_idat;
    uint32_t done = 0;
    bool sound = true;
    for (uint32_t k = 0; k < r.idat_chunks; k++) {
        if (pos + 12 > slot) {
            sound = false;
            break;
        }
        uint32_t len = uni(get_be32(f + pos));
        if (pos + 12 + len > slot || len > r.idat_bytes - done) {
            sound = false;
            break;
        }
        const uint8_t* s = f + pos + 8;
        uint8_t* d = dst + done;
        uint32_t head = (uint32_t)((0 - reinterpret_cast<uintptr_t>(d)) & 15);
        if (head > len) head = len;
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        const uint32_t blocks = (len - head) / 16;
        for (uint32_t j = threadIdx.x; j < blocks; j += THREADS) {
            const Bytes16 v = *reinterpret_cast<const Bytes16*>(s + head + 16ull * j);
            *reinterpret_cast<uint4*>(d + head + 16ull * j) = make_uint4(v.x, v.y, v.z, v.w);
        }
        const uint32_t at = head + 16 * blocks;
        if (threadIdx.x < len - at) d[at + threadIdx.x] = s[at + threadIdx.x];
        done += len;
        pos += 12ull + len;
    }
    if (threadIdx.x == 0) {  // (an info record that does not describe the file: skipped, like a file the scan refused)
        a.png_status[i] = sound && done == r.idat_bytes ? kPngOk : kPngSkipped;
        a.comp_len[i] = sound && done == r.idat_bytes ? done : 0u;
    }
}

// ---- fdh_png_colour_batch ----
struct ColourArgs {
    const uint8_t* file;
    const uint64_t* file_off;
    const PngInfo* info;
    uint32_t* pal;     // nullable unless colour_type == 3: 256 words per file
    uint32_t* colour;  // 4 words per file
    uint32_t* png_status;
    uint64_t n;
    uint32_t width, bit_depth, colour_type;
};

constexpr uint32_t kTRNS = 0x74524E53u;

// One file per wavefront.  The chunks between IHDR and the first IDAT are walked by all lanes alike (the addresses are
// the same in every lane: scalar loads); the first finding in file order is the status.  Then every lane builds four
// of the 256 palette words.  The scan has been over these chunks: their lengths fit the file and their CRCs are right.
// `r` is the file's record, `ct` its colour type, `st` what the caller's checks of the record found (kPngOk: read).
__device__ __forceinline__ void png_colour_file(const ColourArgs& a, uint64_t i, uint32_t lane, const PngInfo& r, uint32_t ct, uint32_t st) {
    const uint64_t slot = a.file_off[i + 1] - a.file_off[i];
    const uint8_t* f = a.file + a.file_off[i];
    if (st == kPngOk && r.first_idat > slot) st = kPngSkipped;  // (an info record that does not describe the file)
    const uint32_t end = uni(r.first_idat);
    uint64_t pos = 8;
    bool have_plte = false, have_trns = false;
    uint32_t plte_at = 0, count = 0, trns_at = 0, trns_len = 0;
    while (st == kPngOk && pos < end) {
        if (pos + 12 > end) {
            st = kPngSkipped;
            break;
        }
        const uint32_t len = uni(get_be32(f + pos)), type = uni(get_be32(f + pos + 4));
        if (pos + 12 + len > end) {
            st = kPngSkipped;
            break;
        }
        if (type == kPLTE && ct == 3) {
            if (have_plte || len == 0 || len % 3 != 0 || len > 768) st = kPngBadPlte;
            have_plte = true;
            plte_at = (uint32_t)pos + 8;
            count = len / 3;
        } else if (type == kTRNS && (ct == 0 || ct == 2 || ct == 3)) {
            if (have_trns || (ct == 0 && len != 2) || (ct == 2 && len != 6) || (ct == 3 && (!have_plte || len > count))) st = kPngBadTrns;
            have_trns = true;
            trns_at = (uint32_t)pos + 8;
            trns_len = len;
        }
        pos += 12ull + len;
    }
    if (st == kPngOk && ct == 3 && !have_plte) st = kPngBadPlte;
    if (lane == 0) a.png_status[i] = st;
    if (st != kPngOk) return;
    if (lane == 0) {
        const uint8_t* t = f + trns_at;
        const bool key = have_trns && ct != 3;
        uint32_t k[3] = {0, 0, 0};
        for (uint32_t c = 0; key && c < trns_len / 2; c++) k[c] = (uint32_t)t[2 * c] << 8 | t[2 * c + 1];
        uint32_t* w = a.colour + 4 * i;
        w[0] = count;
        w[1] = key ? 1u : 0u;
        w[2] = k[0] | k[1] << 16;
        w[3] = k[2];
    }
    if (ct != 3) return;
    uint32_t e[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t idx = 4 * lane + j;
        uint32_t v = 0xFF000000u;
        if (idx < count) {
            const uint8_t* p = f + plte_at + 3 * idx;
            v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (idx < trns_len ? (uint32_t)f[trns_at + idx] : 255u) << 24;
        }
        e[j] = v;
    }
    const Bytes16 v{e[0], e[1], e[2], e[3]};
    *reinterpret_cast<Bytes16*>(a.pal + 256 * i + 4 * lane) = v;
}

}  // namespace fdh
