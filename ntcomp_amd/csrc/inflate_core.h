// Inflate of gzip members of at most 64 KiB (`--inflate gpu`, ntc_inflate_members): the per-member
// decoder behind the kernel in inflate.hip.  Written once as host + device code, like
// deflate_core.h: inf_member is the kernel's whole body, and the host restatement
// (ntc_inflate_members without a context, tests/inflate_cpu) runs the very same function with one
// lane, so bytes and statuses agree by construction and are checked without a GPU.
//
// Vocabulary.  A member is a gzip header (RFC 1952: FEXTRA, FNAME, FCOMMENT and
// FHCRC skipped or checked as zlib does), any number of deflate blocks (RFC 1951: stored, fixed,
// dynamic, in any mix) and the trailer (CRC-32, ISIZE).  It must fill src[0, src_bytes) exactly and
// inflate to exactly claimed_out <= kInfMaxOut bytes.  The output is assembled in a window in LDS
// and copied to dst only when every check has passed: a member that fails writes nothing.
//
// Per deflate block: lane 0 parses the block header and the code-length sequence; all lanes build
// the two decode tables (counts per length, first codes, a direct-lookup table for codes of at
// most kInfRoot bits and the symbols in canonical order for the longer ones); then, round by
// round, all lanes stage the next piece of the input in LDS, lane 0 decodes up to kInfQueue tokens
// into a queue with their output offsets, and the wave executes the queue: literals side by side,
// matches in order, each copied by all lanes as win[p + j] = win[p - d + j mod d].
//
// The input is an arbitrary file.  No lane reads outside src[0, src_bytes) (the bit reader gives
// zeros past the end, and a failure found with the cursor past the end is an input overrun), none
// writes outside win[0, claimed_out) (every token is checked before it is queued), and every
// round consumes input or ends the member.  The code is written for `nl` lanes as deflate_core.h
// is; the host runs it with lane = 0, nl = 1, and nothing in the result depends on nl.
#pragma once
#include "deflate_core.h"

namespace ntc {

constexpr uint32_t kInfMaxOut = 65536;  // the most bytes a member may inflate to (BGZF: 65,280 by convention)
constexpr uint32_t kInfQueue = 64;      // tokens per round
constexpr uint32_t kInfIn = 1024;       // bytes of input staged per phase
constexpr uint32_t kInfRoot = 10;       // bits of the direct-lookup tables
// a phase never needs more staged input than this: a dynamic header is at most 14 + 19 * 3 +
// 316 * (7 + 7) bits = 563 bytes, a round of 64 tokens at most 64 * 48 bits = 384 bytes
constexpr uint32_t kInfHeaderIn = 640, kInfRoundIn = 448;
static_assert(kInfHeaderIn <= kInfIn && kInfRoundIn <= kInfIn, "a phase's input fits the staging buffer");

// a member's status (ntc_inflate_result.status)
enum InfStatus : uint32_t {
    kInfOk = 0,
    kInfBadHeader = 1,  // not 1f 8b 08, a reserved flag bit, a header CRC16 that does not match
    kInfBadBlock = 2,   // block type 3, stored LEN != ~NLEN, HLIT > 286, HDIST > 30
    kInfBadCode = 3,    // a code-length, literal/length or distance code zlib's inflate_table refuses, no
                        // end-of-block code, a repeat with nothing before it or past the end, bits that are no
                        // code, length symbols 286/287, distance symbols 30/31
    kInfBadDistance = 4,  // a distance past the bytes produced so far
    kInfOutput = 5,     // a literal, match or stored block past claimed_out
    kInfInput = 6,      // the member does not end at src_bytes: bits needed past it, or bytes left behind the trailer
    kInfCrc = 7,        // the trailer's CRC-32 is not that of the bytes produced
    kInfIsize = 8,      // the trailer's ISIZE is not claimed_out, or not the bytes produced
    kInfTooLarge = 9,   // claimed_out > kInfMaxOut: nothing was looked at
};

struct InfResult {
    uint32_t status, out_bytes, crc, reserved;  // out_bytes and crc: what was produced (0 unless status is 0, 7 or 8)
};

constexpr uint32_t kInfTokMatch = 0x80000000u;  // a token: a literal byte, or bit 31 | length << 16 | distance - 1

// A member's working set: one workgroup's LDS on the device.
struct InfWork {
    alignas(16) uint8_t win[kInfMaxOut];  // the output so far
    alignas(16) uint8_t in[kInfIn];       // src[in_base, in_base + kInfIn)
    uint16_t tab[2][1u << kInfRoot];      // [0] literal/length, [1] distance: symbol | length << 9, 0: no short code
    uint16_t sorted[2][288];              // the symbols in canonical order
    uint32_t count[2][16];                // codes per length
    uint8_t lens[288 + 32];               // code lengths: literal/length, then distance
    uint32_t crc_tab[256], crc_part[64];
    uint32_t q_tok[kInfQueue], q_off[kInfQueue];
    uint32_t first[16], offs[16];         // of the code being built: first code and place in sorted, per length
    uint32_t cl_cnt[8], cl_offs[8], cl_sym[kDfCL];  // the code-length code (lane 0's)
    uint8_t cl_len[kDfCL + 1];
    uint64_t in_base;
    uint32_t n_q;      // tokens in the queue
    uint32_t type, last;  // the block's BTYPE and BFINAL
    uint32_t next_out;    // bytes produced once the queue has run
    uint32_t outp;     // bytes produced
    uint32_t status;   // first failure
    uint32_t done;     // 1: the block ended, 2: it was the last
    uint32_t fixed;    // the tables are the fixed code's
    uint32_t nsym[2];  // symbols of the two codes of this block
    uint32_t st_src, st_len;  // a stored block's bytes
    uint64_t bitpos;   // the cursor
};

// The bit cursor of lane 0 over the staged input.
struct InfBits {
    const InfWork *W;
    uint64_t src_bytes;
    uint64_t buf;
    uint32_t cnt;
    uint64_t next;  // next byte to load
};
DF_HD uint32_t inf_byte(const InfBits &b, uint64_t p) {
    if (p >= b.src_bytes) return 0;
    const uint64_t i = p - b.W->in_base;
    return i < kInfIn ? b.W->in[i] : 0;  // (never outside a phase's budget: see kInfHeaderIn)
}
DF_HD void inf_open(InfBits &b, const InfWork *W, uint64_t src_bytes) {
    b.W = W, b.src_bytes = src_bytes, b.buf = 0, b.cnt = 0, b.next = W->bitpos >> 3;
    const uint32_t skip = (uint32_t)(W->bitpos & 7);
    b.buf = inf_byte(b, b.next++) >> skip;
    b.cnt = 8 - skip;
}
DF_HD void inf_fill(InfBits &b) {  // at least 56 bits
    while (b.cnt <= 56) {
        b.buf |= (uint64_t)inf_byte(b, b.next++) << b.cnt;
        b.cnt += 8;
    }
}
DF_HD uint32_t inf_get(InfBits &b, uint32_t k) {  // k <= 16, after inf_fill
    const uint32_t v = (uint32_t)(b.buf & ((1u << k) - 1));
    b.buf >>= k, b.cnt -= k;
    return v;
}
DF_HD uint64_t inf_pos(const InfBits &b) { return b.next * 8 - b.cnt; }

// all lanes: src[at, at + n) into W->in (n <= kInfIn), zeros past the end
DF_HD void inf_stage(InfWork *W, const uint8_t *src, uint64_t src_bytes, uint32_t n, uint32_t lane, uint32_t nl) {
    DF_SYNC();  // (the cursor is written, the last phase's readers are done)
    const uint64_t at = W->bitpos >> 3;
    for (uint32_t i = lane; i < n; i += nl) W->in[i] = at + i < src_bytes ? src[at + i] : 0;
    if (lane == 0) W->in_base = at;
    DF_SYNC();
}

// lane 0: end the member.  A failure with the cursor past the input is an input overrun.
DF_HD void inf_fail(InfWork *W, uint32_t kind, uint64_t bitpos, uint64_t src_bytes) {
    if (!W->status) W->status = bitpos > src_bytes * 8 ? (uint32_t)kInfInput : kind;
}

// length symbol 257..285 -> base and extra bits; distance symbol 0..29 likewise
DF_HD uint32_t inf_len_base(uint32_t s, uint32_t *eb) {
    if (s < 265 || s == 285) return *eb = 0, s == 285 ? 258 : s - 254;
    const uint32_t e = (s - 261) / 4;
    return *eb = e, 3 + ((4 + (s - 261) % 4) << e);
}
DF_HD uint32_t inf_dist_base(uint32_t s, uint32_t *eb) {
    if (s < 4) return *eb = 0, s + 1;
    const uint32_t e = s / 2 - 1;
    return *eb = e, 1 + ((2 + (s & 1)) << e);
}

// One symbol of code t (0 literal/length, 1 distance) from the low 15 bits `bits`; *len = its
// length, 0 when the bits are no code.
DF_HD uint32_t inf_decode(const InfWork *W, uint32_t t, uint32_t bits, uint32_t *len) {
    const uint32_t e = W->tab[t][bits & ((1u << kInfRoot) - 1)];
    if (e >> 9) return *len = e >> 9, e & 511;
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        code |= (int32_t)((bits >> (l - 1)) & 1);
        const int32_t c = (int32_t)W->count[t][l];
        if (code - c < first) return *len = l, W->sorted[t][index + (code - first)];
        index += c, first += c;
        first <<= 1, code <<= 1;
    }
    return *len = 0, 0;
}

// All lanes: the decode tables of code t from lens[0, n) (every length <= 15).  What zlib's
// inflate_table refuses is kInfBadCode: an over-subscribed code; an incomplete one unless it is a
// single code of length 1; no code at all, for the literal/length code.
DF_HD void inf_build(InfWork *W, uint32_t t, const uint8_t *lens, uint32_t n, uint64_t src_bytes, uint32_t lane,
                     uint32_t nl) {
    for (uint32_t i = lane; i < 16; i += nl) W->count[t][i] = 0;
    for (uint32_t i = lane; i < (1u << kInfRoot); i += nl) W->tab[t][i] = 0;
    DF_SYNC();
    for (uint32_t s = lane; s < n; s += nl) DF_ADD(&W->count[t][lens[s]], 1u);
    DF_SYNC();
    if (lane == 0) {
        int32_t left = 1;
        uint32_t maxl = 0, code = 0, at = 0;
        bool over = false;
        for (uint32_t l = 1; l <= 15; l++) {
            const uint32_t c = W->count[t][l];
            left = (left << 1) - (int32_t)c;
            if (left < 0) over = true, left = 0;
            if (c) maxl = l;
            W->first[l] = code, W->offs[l] = at;
            code = (code + c) << 1, at += c;
        }
        if (over || (maxl == 0 ? t == 0 : (left > 0 && maxl != 1))) inf_fail(W, kInfBadCode, W->bitpos, src_bytes);
    }
    DF_SYNC();
    if (W->status) return;  // (written before the barrier, not again before the next one: the same for every lane)
    for (uint32_t s = lane; s < n; s += nl) {
        const uint32_t l = lens[s];
        if (!l) continue;
        uint32_t k = 0;
        for (uint32_t u = 0; u < s; u++) k += lens[u] == l;
        W->sorted[t][W->offs[l] + k] = (uint16_t)s;
        if (l <= kInfRoot) {
            const uint16_t e = (uint16_t)(s | l << 9);
            for (uint32_t x = df_rev(W->first[l] + k, l); x < (1u << kInfRoot); x += 1u << l) W->tab[t][x] = e;
        }
    }
    DF_SYNC();
}

// Inflate the member src[0, src_bytes) into dst[0, claimed_out); *res says how it went.  dst is
// written only under status 0.
DF_HD void inf_member(InfWork *W, const uint8_t *src, uint32_t src_bytes, uint32_t claimed_out, uint8_t *dst,
                      InfResult *res, uint32_t lane, uint32_t nl) {
    if (claimed_out > kInfMaxOut) {
        if (lane == 0) res->status = kInfTooLarge, res->out_bytes = 0, res->crc = 0, res->reserved = 0;
        return;
    }
    for (uint32_t i = lane; i < 256; i += nl) W->crc_tab[i] = df_crc_entry(i);
    if (lane == 0) W->status = 0, W->outp = 0, W->fixed = 0, W->done = 0, W->bitpos = 0, W->in_base = 0;
    DF_SYNC();
    // ---- the gzip header (lane 0, from the member itself: a few bytes)
    if (lane == 0) {
        uint64_t p = 10;
        uint32_t st = 0;
        if (src_bytes < 18) st = kInfInput;
        else if (src[0] != 0x1f || src[1] != 0x8b || src[2] != 8 || (src[3] & 0xE0)) st = kInfBadHeader;
        else {
            const uint32_t flg = src[3];
            if (flg & 4) {  // FEXTRA
                if (p + 2 > src_bytes) st = kInfInput;
                else p += 2 + ((uint64_t)src[p] | (uint64_t)src[p + 1] << 8);
            }
            for (uint32_t f = 8; f <= 16 && !st; f <<= 1) {  // FNAME, FCOMMENT: up to and with their zero byte
                if (!(flg & f)) continue;
                while (p < src_bytes && src[p]) p++;
                p++;
            }
            if (!st && (flg & 2)) {  // FHCRC: the low half of the CRC-32 of the header so far
                if (p + 2 > src_bytes) st = kInfInput;
                else {
                    uint32_t c = 0xFFFFFFFFu;
                    for (uint64_t i = 0; i < p; i++) c = W->crc_tab[(c ^ src[i]) & 0xFF] ^ (c >> 8);
                    if (((~c) & 0xFFFF) != ((uint32_t)src[p] | (uint32_t)src[p + 1] << 8)) st = kInfBadHeader;
                    p += 2;
                }
            }
            if (!st && p > src_bytes) st = kInfInput;
        }
        W->status = st;
        W->bitpos = p * 8;
    }
    DF_SYNC();
    // ---- the deflate blocks.  Each one consumes at least 3 bits, so the cursor bounds the loop.
    while (!W->status && W->done != 2) {
        inf_stage(W, src, src_bytes, kInfHeaderIn, lane, nl);
        if (lane == 0) {  // the block header, and a dynamic block's code lengths
            InfBits b;
            inf_open(b, W, src_bytes);
            inf_fill(b);
            const uint32_t last = inf_get(b, 1), type = inf_get(b, 2);
            W->done = 0, W->type = type, W->last = last, W->st_len = 0;
            if (type == 3) inf_fail(W, kInfBadBlock, inf_pos(b), src_bytes);
            else if (type == 0) {
                const uint64_t at = (inf_pos(b) + 7) / 8;  // LEN and NLEN follow the next byte boundary
                if (at + 4 > src_bytes) inf_fail(W, kInfInput, at * 8 + 32, src_bytes);
                else {
                    const uint32_t len = (uint32_t)src[at] | (uint32_t)src[at + 1] << 8;
                    const uint32_t nlen = (uint32_t)src[at + 2] | (uint32_t)src[at + 3] << 8;
                    if ((len ^ nlen) != 0xFFFF) inf_fail(W, kInfBadBlock, at * 8 + 32, src_bytes);
                    else if (at + 4 + len > src_bytes) inf_fail(W, kInfInput, (at + 4 + len) * 8, src_bytes);
                    else if (W->outp + len > claimed_out) inf_fail(W, kInfOutput, at * 8 + 32, src_bytes);
                    else {
                        W->st_src = (uint32_t)(at + 4), W->st_len = len;
                        W->bitpos = (at + 4 + len) * 8;
                        W->done = last ? 2 : 1;
                    }
                }
            } else if (type == 1) {
                W->bitpos = inf_pos(b);
                W->nsym[0] = 288, W->nsym[1] = 32;
            } else {
                const uint32_t hlit = inf_get(b, 5) + 257, hdist = inf_get(b, 5) + 1, hclen = inf_get(b, 4) + 4;
                W->fixed = 0;
                if (hlit > 286 || hdist > 30) inf_fail(W, kInfBadBlock, inf_pos(b), src_bytes);
                else {
                    // the code-length code: 19 symbols of at most 7 bits, decoded by counting (at most
                    // 316 symbols follow, so the canonical walk is cheap enough)
                    uint8_t *cl = W->cl_len;
                    uint32_t *cnt = W->cl_cnt, *sym = W->cl_sym, *offs = W->cl_offs;
                    for (uint32_t i = 0; i < kDfCL; i++) cl[i] = 0;
                    for (uint32_t i = 0; i < 8; i++) cnt[i] = 0;
                    for (uint32_t i = 0; i < hclen; i++) {
                        inf_fill(b);
                        cl[df_cl_order(i)] = (uint8_t)inf_get(b, 3);
                    }
                    for (uint32_t i = 0; i < kDfCL; i++) cnt[cl[i]]++;
                    cnt[0] = 0;
                    int32_t left = 1;
                    offs[0] = offs[1] = 0;
                    for (uint32_t l = 1; l <= 7; l++) {
                        left = (left << 1) - (int32_t)cnt[l];
                        if (left < 0) break;
                        if (l < 7) offs[l + 1] = offs[l] + cnt[l];
                    }
                    if (left != 0) inf_fail(W, kInfBadCode, inf_pos(b), src_bytes);  // over-subscribed or incomplete
                    else {
                        for (uint32_t i = 0; i < kDfCL; i++)
                            if (cl[i]) sym[offs[cl[i]]++] = i;
                        const uint32_t total = hlit + hdist;
                        uint32_t i = 0;
                        bool ok = true;
                        while (i < total && ok) {
                            inf_fill(b);
                            int32_t code = 0, first = 0, index = 0;
                            uint32_t s = kDfNone;
                            for (uint32_t l = 1; l <= 7; l++) {
                                code |= (int32_t)((b.buf >> (l - 1)) & 1);
                                const int32_t c = (int32_t)cnt[l];
                                if (code - c < first) {
                                    s = sym[index + (code - first)];
                                    inf_get(b, l);
                                    break;
                                }
                                index += c, first += c;
                                first <<= 1, code <<= 1;
                            }
                            if (s == kDfNone) ok = false;  // (a complete code: only past the input's end)
                            else if (s < 16) W->lens[i++] = (uint8_t)s;
                            else {
                                uint32_t rep, v = 0;
                                if (s == 16) {
                                    if (i == 0) {
                                        ok = false;
                                        break;
                                    }
                                    v = W->lens[i - 1];
                                    rep = 3 + inf_get(b, 2);
                                } else
                                    rep = s == 17 ? 3 + inf_get(b, 3) : 11 + inf_get(b, 7);
                                if (i + rep > total) ok = false;
                                else
                                    while (rep--) W->lens[i++] = (uint8_t)v;
                            }
                        }
                        if (!ok || W->lens[256] == 0) inf_fail(W, kInfBadCode, inf_pos(b), src_bytes);
                        else {
                            // the distance lengths move to their own place behind the literal/length ones
                            for (uint32_t d = hdist; d-- > 0;) W->lens[288 + d] = W->lens[hlit + d];
                            W->nsym[0] = hlit, W->nsym[1] = hdist;
                        }
                    }
                }
                W->bitpos = inf_pos(b);
                if (!W->status && W->bitpos > src_bytes * 8) W->status = kInfInput;
            }
        }
        DF_SYNC();
        if (W->status) break;
        const uint32_t type = W->type, last = W->last;
        if (type == 0) {  // a stored block: a wave-wide copy
            const uint32_t at = W->st_src, len = W->st_len, p = W->outp;
            for (uint32_t i = lane; i < len; i += nl) W->win[p + i] = src[at + i];
            DF_SYNC();
            if (lane == 0) W->outp = p + len;
            DF_SYNC();
            continue;
        }
        if (type == 1 && !W->fixed) {
            for (uint32_t s = lane; s < 288; s += nl) W->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            for (uint32_t s = lane; s < 32; s += nl) W->lens[288 + s] = 5;
            DF_SYNC();
        }
        if (type == 2 || !W->fixed) {
            inf_build(W, 0, W->lens, W->nsym[0], src_bytes, lane, nl);
            inf_build(W, 1, W->lens + 288, W->nsym[1], src_bytes, lane, nl);
            if (lane == 0) W->fixed = type == 1;
            DF_SYNC();
            if (W->status) break;
        }
        // ---- rounds of at most kInfQueue tokens.  Each one consumes at least a bit or ends the block.
        while (!W->status && !W->done) {
            inf_stage(W, src, src_bytes, kInfRoundIn, lane, nl);
            if (lane == 0) {
                InfBits b;
                inf_open(b, W, src_bytes);
                uint32_t nq = 0, outp = W->outp;
                while (nq < kInfQueue) {
                    inf_fill(b);
                    uint32_t l;
                    const uint32_t s = inf_decode(W, 0, (uint32_t)b.buf & 0x7FFF, &l);
                    if (!l || s > 285) {
                        inf_fail(W, kInfBadCode, inf_pos(b) + (l ? l : 1), src_bytes);
                        break;
                    }
                    inf_get(b, l);
                    if (s < 256) {
                        if (outp >= claimed_out) {
                            inf_fail(W, kInfOutput, inf_pos(b), src_bytes);
                            break;
                        }
                        W->q_tok[nq] = s, W->q_off[nq++] = outp++;
                        continue;
                    }
                    if (s == 256) {
                        W->done = last ? 2 : 1;
                        break;
                    }
                    uint32_t eb;
                    uint32_t len = inf_len_base(s, &eb);
                    len += inf_get(b, eb);
                    const uint32_t ds = inf_decode(W, 1, (uint32_t)b.buf & 0x7FFF, &l);
                    if (!l || ds > 29) {
                        inf_fail(W, kInfBadCode, inf_pos(b) + (l ? l : 1), src_bytes);
                        break;
                    }
                    inf_get(b, l);
                    uint32_t dist = inf_dist_base(ds, &eb);
                    dist += inf_get(b, eb);
                    if (dist > outp) {
                        inf_fail(W, kInfBadDistance, inf_pos(b), src_bytes);
                        break;
                    }
                    if (outp + len > claimed_out) {
                        inf_fail(W, kInfOutput, inf_pos(b), src_bytes);
                        break;
                    }
                    W->q_tok[nq] = kInfTokMatch | len << 16 | (dist - 1), W->q_off[nq++] = outp;
                    outp += len;
                }
                W->bitpos = inf_pos(b);
                if (!W->status && W->bitpos > src_bytes * 8) W->status = kInfInput;
                W->n_q = W->status ? 0 : nq;  // a failed member's output is not needed
                W->next_out = outp;
            }
            DF_SYNC();
            const uint32_t nq = W->n_q;
            for (uint32_t i = lane; i < nq; i += nl) {
                const uint32_t t = W->q_tok[i];
                if (!(t & kInfTokMatch)) W->win[W->q_off[i]] = (uint8_t)t;
            }
            DF_SYNC();
            for (uint32_t i = 0; i < nq; i++) {
                const uint32_t t = W->q_tok[i];
                if (!(t & kInfTokMatch)) continue;
                const uint32_t p = W->q_off[i], len = (t >> 16) & 0x1FF, d = (t & 0x7FFF) + 1;
                const uint32_t from = p - d;
                if (d >= len)
                    for (uint32_t j = lane; j < len; j += nl) W->win[p + j] = W->win[from + j];
                else
                    for (uint32_t j = lane; j < len; j += nl) W->win[p + j] = W->win[from + j % d];
                DF_SYNC();
            }
            if (lane == 0) W->outp = W->next_out;
            DF_SYNC();
        }
    }
    DF_SYNC();
    // ---- the trailer: CRC-32 (a piece per lane, joined by lane 0) and ISIZE
    const uint32_t n = W->outp;
    const uint32_t piece = (n + nl - 1) / nl;
    if (!W->status) {
        const uint32_t a = lane * piece < n ? lane * piece : n, e = a + piece < n ? a + piece : n;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = a; i < e; i++) c = W->crc_tab[(c ^ W->win[i]) & 0xFF] ^ (c >> 8);
        if (lane < 64) W->crc_part[lane] = ~c;
    }
    DF_SYNC();
    if (lane == 0) {
        uint32_t crc = 0;
        if (!W->status) {
            crc = W->crc_part[0];
            const uint32_t xp = df_gf_xpow8(piece);
            for (uint32_t l = 1; l < nl && l * piece < n; l++) {
                const uint32_t len = n - l * piece < piece ? n - l * piece : piece;
                crc = df_crc_join(crc, W->crc_part[l], len == piece ? xp : df_gf_xpow8(len));
            }
            const uint64_t at = (W->bitpos + 7) / 8;
            if (at + 8 > src_bytes) W->status = kInfInput;
            else {
                uint32_t want = 0, isize = 0;
                for (uint32_t i = 0; i < 4; i++) want |= (uint32_t)src[at + i] << (8 * i), isize |= (uint32_t)src[at + 4 + i] << (8 * i);
                if (want != crc) W->status = kInfCrc;
                else if (isize != n || isize != claimed_out) W->status = kInfIsize;
                else if (at + 8 != src_bytes) W->status = kInfInput;
            }
        }
        const uint32_t st = W->status;
        const bool made = st == kInfOk || st == kInfCrc || st == kInfIsize;
        res->status = st, res->out_bytes = made ? n : 0, res->crc = made ? crc : 0, res->reserved = 0;
    }
    DF_SYNC();
    if (W->status) return;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        struct V16 {
            uint32_t x[4];
        };
        const V16 *s16 = reinterpret_cast<const V16 *>(W->win);
        V16 *d16 = reinterpret_cast<V16 *>(dst);
        for (uint32_t i = lane; i < n / 16; i += nl) d16[i] = s16[i];
        for (uint32_t i = (n & ~15u) + lane; i < n; i += nl) dst[i] = W->win[i];
    } else {
        for (uint32_t i = lane; i < n; i += nl) dst[i] = W->win[i];
    }
}

// Host restatement: one member, one lane.
inline void inf_member_host(const uint8_t *src, uint32_t src_bytes, uint32_t claimed_out, uint8_t *dst, InfResult *res) {
    InfWork *W = new InfWork;
    inf_member(W, src, src_bytes, claimed_out, dst, res, 0, 1);
    delete W;
}

}  // namespace ntc
