// Quality smoothing inside long reference matches: the per-read logic of k_q_smooth in
// quality.hip (DESIGN.md "Smoothing qualities inside long matches").  Written once as host +
// device code, like quality_core.h: the kernel calls these functions, and a CPU program
// (tests/qsmooth_cpu) compiles the very same functions with a host compiler.
//
// Vocabulary: a read of n bases has its records in archive order, rightmost first, with
// lengths L_0 .. L_{m-1} summing to n; record j covers positions [e_j - L_j, e_j), e_0 = n,
// e_{j+1} = e_j - L_j.  A record is long when flag bit 1 of its byte 7 is clear.  A position
// is trusted iff it lies in a long record of at least M bases (M >= 12).  A trusted quality
// above the floor becomes the target; every other byte stays.
//
// The records are taken kQsChunk at a time.  A chunk covers the positions [lo, lo + span) of
// the read; its entry j is record j's first position relative to lo (descending in j, the
// last is 0) with kQsTrusted set for a trusted record.  A record holds fewer than 2^24 bases,
// so a chunk's span stays below 2^30 however long the read is.
#pragma once
#include <cstdint>

#include "quality_core.h"

namespace ntc {

constexpr uint32_t kQsChunk = 64;
constexpr uint32_t kQsTrusted = 1u << 31;
constexpr int64_t kQsMinM = 12, kQsMaxM = 0xFFFFFF;  // the "quality_smooth" option: 0 or kQsMinM .. kQsMaxM
constexpr int64_t kQsToLo = '$', kQsToHi = '~', kQsToDefault = 'I';  // "quality_smooth_to"

Q_HD uint32_t qs_rec_len(uint64_t rec) {
    const uint32_t flag = (uint32_t)(rec >> 56);
    return (flag & 2) ? flag >> 2 : (uint32_t)(rec >> 32) & 0xFFFFFFu;
}

Q_HD bool qs_rec_trusted(uint64_t rec, uint32_t m) { return !((rec >> 56) & 2) && qs_rec_len(rec) >= m; }

// the floor and the target of a mode: the images of '#' and of the option's byte
Q_HD uint32_t qs_floor(uint32_t mode) { return q_table(mode, '#'); }
Q_HD uint32_t qs_target(uint32_t mode, uint32_t to) { return q_table(mode, to); }

// entry of a record: span = the chunk's bases, incl = the lengths of the chunk's records up
// to and including this one
Q_HD uint32_t qs_entry(uint32_t span, uint32_t incl, uint64_t rec, uint32_t m) {
    return (span - incl) | (qs_rec_trusted(rec, m) ? kQsTrusted : 0);
}

// the entries of a chunk, one record after the other (the kernel scans across the wave);
// returns the span
Q_HD uint32_t qs_chunk_entries(const uint64_t *recs, uint32_t cnt, uint32_t m, uint32_t *ent) {
    uint32_t span = 0, incl = 0;
    for (uint32_t j = 0; j < cnt; j++) span += qs_rec_len(recs[j]);
    for (uint32_t j = 0; j < cnt; j++) {
        incl += qs_rec_len(recs[j]);
        ent[j] = qs_entry(span, incl, recs[j], m);
    }
    return span;
}

// 0xFF in bytes [lo, hi) of a word, 0 <= lo < hi <= 8
Q_HD uint64_t qs_bytes(uint32_t lo, uint32_t hi) {
    return (hi >= 8 ? ~0ull : (1ull << (8 * hi)) - 1) & ~((1ull << (8 * lo)) - 1);
}

// The trusted bytes of the 8-byte word whose byte 0 is position p0 of the chunk (negative
// where the word starts before it).  *live: the bytes that are positions of the chunk.
// cnt >= 1, entries as above.
Q_HD uint64_t qs_word_mask(const uint32_t *ent, uint32_t cnt, uint32_t span, int64_t p0, uint64_t *live) {
    const int64_t lo = p0 > 0 ? p0 : 0, hi = p0 + 8 < (int64_t)span ? p0 + 8 : (int64_t)span;
    *live = 0;
    if (lo >= hi) return 0;
    *live = qs_bytes((uint32_t)(lo - p0), (uint32_t)(hi - p0));
    uint32_t a = 0, b = cnt - 1;  // the first record that starts at or before lo (the last starts at 0)
    while (a < b) {
        const uint32_t mid = (a + b) / 2;
        if ((int64_t)(ent[mid] & ~kQsTrusted) <= lo) b = mid;
        else a = mid + 1;
    }
    uint64_t mask = 0;
    int64_t s = lo;
    for (uint32_t j = a;; j--) {  // towards the read's end: record j ends where record j - 1 starts
        int64_t e = j ? (int64_t)(ent[j - 1] & ~kQsTrusted) : (int64_t)span;
        if (e > hi) e = hi;
        if (e > s) {
            if (ent[j] & kQsTrusted) mask |= qs_bytes((uint32_t)(s - p0), (uint32_t)(e - p0));
            s = e;
        }
        if (s >= hi || j == 0) break;
    }
    return mask;
}

// The word after the rule: a byte under mask that exceeds the floor becomes the target.
// *changed: 0xFF in every byte the rule replaced (also where it already held the target).
Q_HD uint64_t qs_apply(uint64_t v, uint64_t mask, uint32_t floor, uint32_t target, uint64_t *changed) {
    // all eight bytes at once: with bit 7 set in every byte no borrow crosses a byte, and bit 7
    // of byte - (floor + 1) survives iff the byte (of '!'..'~' where it counts) exceeds the floor
    const uint64_t ones = 0x0101010101010101ull, high = ones << 7;
    const uint64_t above = (((v & ~high) | high) - ones * (floor + 1)) & high;
    const uint64_t ch = (above >> 7) * 0xFF & mask;
    *changed = ch;
    return (v & ~ch) | (ch & (0x0101010101010101ull * target));
}

// the live bytes of a word into a presence map
Q_HD void qs_presence(uint64_t v, uint64_t live, uint64_t *p0, uint64_t *p1) {
    for (uint32_t j = 0; j < 8; j++) {
        if (!((live >> (8 * j)) & 1)) continue;
        const uint32_t c = (uint32_t)(v >> (8 * j)) & 0x7F;
        if (c < 64) *p0 |= 1ull << c;
        else *p1 |= 1ull << (c - 64);
    }
}

}  // namespace ntc
