// BGZF output (`decode --bgzf`, ntc_bgzf_compress): the member plan, one rule for
// the host and the device.  A text of n bytes, with or without record offsets off[0..R], is cut
// into members of at most kBgzfMember bytes; a member is chunks for deflate_core.h's
// df_code_chunk, coded on their own and joined behind a BGZF header.  bgzf.hip runs the rule with
// one lane per grid point or member, bgzf_host below walks it serially: both call bgzf_cut,
// bgzf_cell_counts, bgzf_member_at and bgzf_chunk_at, so the tables agree by construction.
//
// Without offsets the cuts are the multiples of kBgzfMember.  With offsets cut_j is the largest
// off[r] <= j kBgzfGrid, for j = 0 .. ceil(n / kBgzfGrid); cell j = [cut_j, cut_j+1) yields
// ceil(L / kBgzfMember) members, all of kBgzfMember bytes but the last.  A cell is shorter than
// the grid step plus the record lying over its left grid point, so members end on record
// boundaries unless a record is longer than kBgzfMember - kBgzfGrid + 1 bytes.
#pragma once
#include <vector>

#include "deflate_core.h"

namespace ntc {

constexpr uint32_t kBgzfMember = 65280;  // M: input bytes per member at most (bgzip's value)
constexpr uint32_t kBgzfGrid = 61440;    // G: grid step of the record-aligned cuts
constexpr uint32_t kBgzfHeader = 18, kBgzfTrailer = 8;
constexpr uint32_t kBgzfMemberChunks = (kBgzfMember + kDfChunk - 1) / kDfChunk;  // 2: 32,768 bytes, then the rest
// a member of L bytes is at most 18 + L + B chunks + 8 bytes (deflate_core.h kDfB), so BSIZE fits
constexpr uint32_t kBgzfSlack = kBgzfHeader + kBgzfTrailer + kDfB * kBgzfMemberChunks;  // 36
static_assert(kBgzfMember + kBgzfSlack <= 65536, "BSIZE = member bytes - 1 is a u16");
static_assert(kBgzfGrid < kBgzfMember, "a cell of short records is one member");

// (text offset, text bytes, place in the output, bytes there): ntc_bgzf_member's layout
struct BgzfMember {
    uint64_t text_off, text_bytes, place, bytes;
};

DF_HD uint8_t bgzf_header_byte(uint32_t i) {  // the 16 bytes before BSIZE
    return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xff : i == 10 ? 6 : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2 : 0;
}
constexpr uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

DF_HD uint64_t bgzf_cells(uint64_t n, bool records) {
    const uint64_t step = records ? kBgzfGrid : kBgzfMember;
    return (n + step - 1) / step;
}
// the most members the rule makes of n bytes, whatever the offsets: a cell of L bytes yields at
// most L / M + 1, and there are ceil(n / G) cells
DF_HD uint64_t bgzf_members_max(uint64_t n) { return (n + kBgzfGrid - 1) / kBgzfGrid + n / kBgzfMember; }
DF_HD uint64_t bgzf_bound(uint64_t n) { return n + (uint64_t)kBgzfSlack * bgzf_members_max(n); }

// cut j of the text; off (null: plain cuts) holds n_rec + 1 offsets, off[r] - base being record
// r's start in the text (base = off[0])
DF_HD uint64_t bgzf_cut(const uint64_t *off, uint64_t n_rec, uint64_t base, uint64_t n, uint64_t j) {
    if (!off) return j * kBgzfMember < n ? j * kBgzfMember : n;
    const uint64_t x = j * kBgzfGrid;
    if (x >= n) return n;  // (off[n_rec] = n is then the largest)
    uint64_t lo = 0, hi = n_rec;  // off[lo] - base <= x throughout
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] - base <= x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return off[lo] - base;
}
DF_HD uint32_t bgzf_chunks_of(uint64_t len) { return (uint32_t)((len + kDfChunk - 1) / kDfChunk); }  // len > 0
// members and chunks of a cell of L bytes, packed members << 32 | chunks
DF_HD uint64_t bgzf_cell_counts(uint64_t L) {
    if (!L) return 0;
    const uint64_t m = (L + kBgzfMember - 1) / kBgzfMember, last = L - (m - 1) * kBgzfMember;
    return m << 32 | ((m - 1) * kBgzfMemberChunks + bgzf_chunks_of(last));
}
// member i of the cell [a, b): its text and its first chunk, given the cell's first chunk
DF_HD void bgzf_member_at(uint64_t a, uint64_t b, uint64_t i, uint64_t cell_chunk0, uint64_t *start, uint32_t *len, uint64_t *chunk0) {
    *start = a + i * kBgzfMember;
    *len = (uint32_t)(b - *start < kBgzfMember ? b - *start : kBgzfMember);
    *chunk0 = cell_chunk0 + i * kBgzfMemberChunks;
}
// chunk c of a member of len bytes at start: its place and bytes
DF_HD void bgzf_chunk_at(uint64_t start, uint32_t len, uint32_t c, uint64_t *src_off, uint32_t *n, uint32_t *last) {
    *src_off = start + (uint64_t)c * kDfChunk;
    *n = len - c * kDfChunk < kDfChunk ? len - c * kDfChunk : kDfChunk;
    *last = c + 1 == bgzf_chunks_of(len);
}

// a member's 18 header bytes and its trailer, around chunk bytes that are `body` long
DF_HD void bgzf_frame(uint8_t *o, uint32_t body, uint32_t crc, uint32_t isize) {
    const uint32_t bsize = kBgzfHeader + body + kBgzfTrailer - 1;
    for (uint32_t i = 0; i < 16; i++) o[i] = bgzf_header_byte(i);
    o[16] = (uint8_t)bsize, o[17] = (uint8_t)(bsize >> 8);
    uint8_t *t = o + kBgzfHeader + body;
    for (uint32_t i = 0; i < 4; i++) t[i] = (uint8_t)(crc >> (8 * i)), t[4 + i] = (uint8_t)(isize >> (8 * i));
}

// Host restatement: the rule above walked serially, df_code_chunk with one lane.  out: room for
// bgzf_bound(n) bytes; tab gets the member table; counts: members, chunks, text bytes, bytes,
// chunks stored / Huffman / Huffman with matches (added to, but for the four totals).
inline void bgzf_host(const uint8_t *text, uint64_t n, const uint64_t *off, uint64_t n_rec, uint8_t *out, std::vector<BgzfMember> &tab,
               uint64_t counts[7]) {
    DfWork *W = new DfWork;
    std::vector<uint32_t> tokens(kDfChunk);
    std::vector<uint8_t> slot(kDfSlot);
    uint64_t at = 0;
    const uint64_t cells = bgzf_cells(n, off != nullptr);
    for (uint64_t j = 0; j < cells; j++) {
        const uint64_t a = bgzf_cut(off, n_rec, 0, n, j), b = bgzf_cut(off, n_rec, 0, n, j + 1);
        for (uint64_t i = 0; i < bgzf_cell_counts(b - a) >> 32; i++) {
            uint64_t start, chunk0;
            uint32_t len, body = 0, crc = 0;
            bgzf_member_at(a, b, i, 0, &start, &len, &chunk0);
            for (uint32_t c = 0; c < bgzf_chunks_of(len); c++) {
                uint64_t src;
                uint32_t m, last;
                bgzf_chunk_at(start, len, c, &src, &m, &last);
                DfResult r{};
                df_code_chunk(W, text + src, m, last != 0, tokens.data(), slot.data(), &r, 0, 1);
                std::memcpy(out + at + kBgzfHeader + body, slot.data(), r.size);
                body += r.size;
                crc = c ? df_crc_join(crc, r.crc, df_gf_xpow8(m)) : r.crc;
                counts[1]++;
                counts[3 + r.choice]++;
            }
            bgzf_frame(out + at, body, crc, len);
            tab.push_back(BgzfMember{start, len, at, (uint64_t)kBgzfHeader + body + kBgzfTrailer});
            at += tab.back().bytes;
        }
    }
    delete W;
    counts[0] = tab.size();
    counts[2] = n;
    counts[3] = at;
}

}  // namespace ntc
