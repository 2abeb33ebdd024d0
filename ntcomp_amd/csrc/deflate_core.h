// Deflate of the packed block streams (`--deflate gpu`, NTC_DEFLATE_GPU): the per-chunk coder
// behind the kernels in deflate.hip.  Written once as host + device code, like qrans_core.h:
// df_code_chunk is the kernel's whole body, and the host restatement (df_member_host below,
// ntc_deflate_stream with engine 3, tests/deflate_cpu) runs the very same function with one
// lane, so the bytes agree by construction and are checked without a GPU.
//
// Vocabulary.  A stream of n bytes is cut into chunks of kDfChunk bytes (an
// empty stream has one empty chunk); a chunk is coded on its own and its output ends on a byte
// boundary, so a member is header + the chunks' bytes back to back + trailer.  Per chunk three
// encodings are costed exactly, in bits, and the cheapest is written, ties to the lower number:
//   1  one stored block;
//   2  one dynamic-Huffman block of literals only;
//   3  one dynamic-Huffman block of literals and matches.
// A chunk that is not the stream's last and is coded as 2 or 3 ends with an empty stored block
// (3 bits, padding, 00 00 ff ff), which the cost includes; the last chunk's block has BFINAL.
//
// The code is written for `nl` lanes that run it side by side: a loop `for (i = lane; i < N;
// i += nl)` shares N items among them, DF_SYNC() separates the phases, and what several lanes
// may touch at once goes through DF_ADD / DF_OR / DF_MAX, whose results do not depend on the
// order of arrival.  The host runs it with lane = 0, nl = 1.  Nothing in the output depends on
// nl: the matcher's step is kDfStep positions whatever the lane count.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ __forceinline__
#else
#define DF_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DF_SYNC() __syncthreads()
#define DF_ADD(p, v) atomicAdd((p), (v))
#define DF_OR(p, v) atomicOr((p), (v))
#define DF_MAX(p, v) atomicMax((p), (v))
#else
#define DF_SYNC() ((void)0)
#define DF_ADD(p, v) (*(p) += (v))
#define DF_OR(p, v) (*(p) |= (v))
#define DF_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#endif

namespace ntc {

#ifndef NTC_DF_CHUNK
#define NTC_DF_CHUNK 32768  // (a build with another value is for measuring C only: DESIGN.md §26)
#endif
constexpr uint32_t kDfChunk = NTC_DF_CHUNK;  // C: input bytes per chunk (<= 32,768: one stored block holds it, every distance is legal)
constexpr uint32_t kDfStep = 64;       // positions the matcher looks at side by side
constexpr uint32_t kDfHashBits = 13;   // buckets of the position table
constexpr uint32_t kDfMinMatch = 3, kDfMaxMatch = 258;
constexpr uint32_t kDfTooFar = 4096;   // a 3-byte match further back than this costs more than 3 literals
constexpr uint32_t kDfLL = 286, kDfD = 30, kDfCL = 19;
constexpr uint32_t kDfNone = 0xFFFFFFFFu;
// B of the size bound.  A chunk of m bytes comes out as at most m + 5 bytes: the stored form is
// exactly m + 5 (one block, as kDfChunk < 65,536), and a Huffman form is written only when its
// cost, 3 + 32 bits of marker included, is below 8 (m + 5) bits; its bytes are the bits before
// the marker's 32 rounded up plus 4, so again at most m + 5.
constexpr uint32_t kDfB = 5;
constexpr uint32_t kDfSlot = kDfChunk + 16;  // bytes of a chunk's slot in the staging buffer
static_assert(kDfChunk <= 32768 && kDfChunk % 16 == 0, "a chunk is one stored block and no distance passes 32,768");

DF_HD uint64_t df_chunks(uint64_t n) { return n ? (n + kDfChunk - 1) / kDfChunk : 1; }
// the most bytes the member of an n-byte stream takes: 18 + n + B ceil(n / C) + 5
DF_HD uint64_t df_member_bound(uint64_t n) { return 18 + n + (uint64_t)kDfB * ((n + kDfChunk - 1) / kDfChunk) + 5; }

// ---- CRC-32 (zlib's polynomial, reflected) ------------------------------------------------
constexpr uint32_t kDfPoly = 0xEDB88320u;
DF_HD uint32_t df_crc_entry(uint32_t i) {
    for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1) ? kDfPoly : 0);
    return i;
}
// a(x) b(x) mod P in the reflected representation (bit 31 = x^0)
DF_HD uint32_t df_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? kDfPoly : 0);
    }
    return p;
}
// x^(8 len) mod P
DF_HD uint32_t df_gf_xpow8(uint64_t len) {
    uint32_t r = 0x80000000u, base = 0x40000000u;  // x^0, x^1
    for (uint64_t e = len * 8; e; e >>= 1) {
        if (e & 1) r = df_gf_mul(r, base);
        base = df_gf_mul(base, base);
    }
    return r;
}
// crc(A || B) from crc(A), crc(B) and x^(8 |B|): zlib's crc32_combine
DF_HD uint32_t df_crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t xpow_b) { return df_gf_mul(xpow_b, crc_a) ^ crc_b; }

// ---- symbols -----------------------------------------------------------------------------
DF_HD uint32_t df_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x != 0
// length 3..258 -> length symbol 257..285, its extra bits and their value
DF_HD uint32_t df_len_sym(uint32_t len, uint32_t *ebits, uint32_t *extra) {
    const uint32_t l = len - 3;
    if (l < 8 || len == 258) {
        *ebits = *extra = 0;
        return len == 258 ? 285 : 257 + l;
    }
    const uint32_t e = df_log2(l) - 2;
    *ebits = e;
    *extra = l & ((1u << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}
// distance 1..32768 -> distance symbol 0..29
DF_HD uint32_t df_dist_sym(uint32_t dist, uint32_t *ebits, uint32_t *extra) {
    const uint32_t d = dist - 1;
    if (d < 4) {
        *ebits = *extra = 0;
        return d;
    }
    const uint32_t n = df_log2(d);
    *ebits = n - 1;
    *extra = d & ((1u << (n - 1)) - 1);
    return 2 * n + ((d >> (n - 1)) & 1);
}
DF_HD uint32_t df_ll_ebits(uint32_t s) { return s < 265 || s == 285 ? 0 : (s - 261) / 4; }
DF_HD uint32_t df_d_ebits(uint32_t s) { return s < 4 ? 0 : s / 2 - 1; }
DF_HD uint32_t df_cl_ebits(uint32_t s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }
// the order in which the code-length code's own lengths are sent
DF_HD uint32_t df_cl_order(uint32_t i) {
    constexpr uint8_t order[kDfCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
DF_HD uint32_t df_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; i++) r |= ((code >> i) & 1) << (len - 1 - i);
    return r;
}

// ---- the matcher's rules -------------------------------------------------------------------
// Positions are looked at in steps of kDfStep.  A position p of a step probes one bucket, the
// one of the three bytes at p, as the steps before left it: the bucket holds the highest
// position below the step's first position whose three bytes hash alike (position + 1; 0: none).
// Its candidate is extended byte by byte to at most 258 and the chunk's end; a match counts
// from 3 bytes, a 3-byte one only up to kDfTooFar back.  Then the step's positions that still
// have three bytes enter the table, the highest winning a bucket, and the cursor walks the
// step: a position with a match emits it and jumps behind it, any other emits its literal.
// Positions the cursor jumped over emit nothing (they still entered the table).
DF_HD uint32_t df_hash(const uint8_t *p) {
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    return (v * 0x9E3779B1u) >> (32 - kDfHashBits);
}
DF_HD uint32_t df_match_len(const uint8_t *d, uint32_t q, uint32_t p, uint32_t n) {
    uint32_t lim = n - p;
    if (lim > kDfMaxMatch) lim = kDfMaxMatch;
    uint32_t m = 0;
    while (m < lim && d[q + m] == d[p + m]) m++;
    return m;
}
// a token: a literal byte, or bit 31 | (distance - 1) << 8 | (length - 3)
constexpr uint32_t kDfTokMatch = 0x80000000u;

struct DfPlan {
    uint32_t bits;  // the encoding's whole cost in bits, the marker included
    uint16_t hlit, hdist, hclen, n_rle;
    uint8_t rle_sym[kDfLL + kDfD + 4], rle_extra[kDfLL + kDfD + 4];
    uint8_t cl_len[32];
};

// A chunk's working set: one workgroup's LDS on the device.
struct DfWork {
    alignas(16) uint8_t data[kDfChunk];
    union {
        uint32_t head[1u << kDfHashBits];  // the position table (matching)
        uint32_t out[kDfChunk / 4 + 8];    // the bits of the encoding (writing)
    } u;
    uint32_t freq_ll[2][288], freq_d[2][32], freq_cl[32];  // [0]: encoding 3, [1]: encoding 2
    uint8_t len_ll[2][288], len_d[2][32];
    uint16_t code_ll[288], code_d[32], code_cl[32];
    uint32_t key[288];
    uint16_t sym[288];
    uint32_t num[34], first[34];
    uint32_t crc_tab[256], crc_part[kDfStep];
    uint16_t step_len[kDfStep], step_dist[kDfStep];
    uint32_t step_off[kDfStep + 1];
    uint32_t step_any[2];  // any match in this step (by step parity: the other one is being cleared)
    uint32_t force[2], n_used;
    uint32_t sc[4];
    DfPlan plan[2];
};

struct DfResult {
    uint32_t size;    // bytes written
    uint32_t crc;     // CRC-32 of the chunk's input
    uint32_t choice;  // 1, 2 or 3
    uint32_t n_tok;   // tokens of encoding 3
};

// OR the low nbits (<= 48) of v into the bit string out at bitpos
DF_HD void df_put(uint32_t *out, uint32_t bitpos, uint64_t v, uint32_t nbits) {
    if (!nbits) return;
    const uint32_t w = bitpos >> 5, sh = bitpos & 31;
    const uint32_t lo = (uint32_t)(v << sh);
    const uint64_t r = (v >> (31 - sh)) >> 1;
    if (lo) DF_OR(&out[w], lo);
    if ((uint32_t)r) DF_OR(&out[w + 1], (uint32_t)r);
    if ((uint32_t)(r >> 32)) DF_OR(&out[w + 2], (uint32_t)(r >> 32));
}

// Code lengths of at most maxbits for the nsym frequencies freq -> lens.  The symbols in use
// are ranked by (frequency, symbol); Moffat and Katajainen's in-place pass over the ranked
// frequencies gives the Huffman depths; the counts per length are repaired to a full code of
// at most maxbits (lengths above it fold into it; while the code is over-subscribed one code of
// maxbits goes, and the deepest shorter length gives one code up for two one bit longer); the
// lengths go out from the shortest to the symbols from the most frequent down.  Like zlib, a
// code never has fewer than two symbols: while fewer are in use, the lowest unused symbol counts
// as seen once (W->force), so every code sent is complete.
DF_HD void df_build_lengths(DfWork *W, const uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *lens,
                            uint32_t lane, uint32_t nl) {
    if (lane == 0) {
        uint32_t used = 0;
        for (uint32_t s = 0; s < nsym; s++) used += freq[s] != 0;
        W->force[0] = W->force[1] = kDfNone;
        for (uint32_t s = 0, k = 0; used < 2; s++)
            if (!freq[s]) W->force[k++] = s, used++;
        W->n_used = used;
    }
    DF_SYNC();
    const uint32_t f0 = W->force[0], f1 = W->force[1];
    for (uint32_t s = lane; s < nsym; s += nl) {
        lens[s] = 0;
        const uint32_t f = freq[s] ? freq[s] : (s == f0 || s == f1);
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < nsym; t++) {
            const uint32_t ft = freq[t] ? freq[t] : (t == f0 || t == f1);
            r += ft && (ft < f || (ft == f && t < s));
        }
        W->key[r] = f;
        W->sym[r] = (uint16_t)s;
    }
    DF_SYNC();
    if (lane == 0) {
        uint32_t *A = W->key;
        const int n = (int)W->n_used;  // >= 2
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < n - 1; next++) {
            if (leaf >= n || A[root] < A[leaf]) {
                A[next] = A[root];
                A[root++] = (uint32_t)next;
            } else
                A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) {
                A[next] += A[root];
                A[root++] = (uint32_t)next;
            } else
                A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2;
        next = n - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) used++, root--;
            while (avbl > used) A[next--] = (uint32_t)dpth, avbl--;
            avbl = 2 * used;
            dpth++;
            used = 0;
        }
        uint32_t *num = W->num;
        for (uint32_t i = 0; i <= maxbits; i++) num[i] = 0;
        for (int i = 0; i < n; i++) num[A[i] < maxbits ? A[i] : maxbits]++;
        uint32_t total = 0;
        for (uint32_t i = maxbits; i > 0; i--) total += num[i] << (maxbits - i);
        while (total != (1u << maxbits)) {
            num[maxbits]--;
            for (uint32_t i = maxbits - 1; i > 0; i--)
                if (num[i]) {
                    num[i]--;
                    num[i + 1] += 2;
                    break;
                }
            total--;
        }
        int j = n;
        for (uint32_t i = 1; i <= maxbits; i++)
            for (uint32_t l = num[i]; l > 0; l--) lens[W->sym[--j]] = (uint8_t)i;
    }
    DF_SYNC();
}

// canonical codes of lens, bit-reversed so that they go out low bit first
DF_HD void df_assign_codes(DfWork *W, const uint8_t *lens, uint32_t nsym, uint32_t maxbits, uint16_t *codes,
                           uint32_t lane, uint32_t nl) {
    if (lane == 0) {
        for (uint32_t i = 0; i <= maxbits; i++) W->num[i] = 0;
        for (uint32_t s = 0; s < nsym; s++) W->num[lens[s]]++;
        uint32_t code = 0;
        W->num[0] = 0;
        W->first[0] = 0;
        for (uint32_t i = 1; i <= maxbits; i++) W->first[i] = code = (code + W->num[i - 1]) << 1;
    }
    DF_SYNC();
    for (uint32_t s = lane; s < nsym; s += nl) {
        const uint32_t len = lens[s];
        uint32_t k = 0;
        for (uint32_t t = 0; t < s; t++) k += lens[t] == len;
        codes[s] = len ? (uint16_t)df_rev(W->first[len] + k, len) : 0;
    }
    DF_SYNC();
}

// Cost encoding 3 (o = 0) or 2 (o = 1) from freq_ll[o] / freq_d[o]: the code lengths, the
// run-length form of the lengths and its code, and plan[o].bits.
DF_HD void df_plan(DfWork *W, uint32_t o, bool last, uint32_t lane, uint32_t nl) {
    DfPlan *P = &W->plan[o];
    df_build_lengths(W, W->freq_ll[o], kDfLL, 15, W->len_ll[o], lane, nl);
    df_build_lengths(W, W->freq_d[o], kDfD, 15, W->len_d[o], lane, nl);
    if (lane == 0) {
        const uint8_t *ll = W->len_ll[o], *dl = W->len_d[o];
        uint32_t hlit = kDfLL, hdist = kDfD;
        while (hlit > 257 && !ll[hlit - 1]) hlit--;
        while (hdist > 1 && !dl[hdist - 1]) hdist--;
        for (uint32_t i = 0; i < kDfCL; i++) W->freq_cl[i] = 0;
        const uint32_t total = hlit + hdist;
        uint32_t nr = 0;
        const auto emit = [&](uint32_t s, uint32_t x) {
            P->rle_sym[nr] = (uint8_t)s;
            P->rle_extra[nr++] = (uint8_t)x;
            W->freq_cl[s]++;
        };
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = i < hlit ? ll[i] : dl[i - hlit];
            uint32_t run = 1;
            while (i + run < total && (i + run < hlit ? ll[i + run] : dl[i + run - hlit]) == v) run++;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const uint32_t r = run < 138 ? run : 138;
                    emit(18, r - 11);
                    run -= r;
                }
                if (run >= 3) emit(17, run - 3), run = 0;
                while (run--) emit(0, 0);
            } else {
                emit(v, 0);
                run--;
                while (run >= 3) {
                    const uint32_t r = run < 6 ? run : 6;
                    emit(16, r - 3);
                    run -= r;
                }
                while (run--) emit(v, 0);
            }
        }
        P->hlit = (uint16_t)hlit;
        P->hdist = (uint16_t)hdist;
        P->n_rle = (uint16_t)nr;
    }
    DF_SYNC();
    df_build_lengths(W, W->freq_cl, kDfCL, 7, P->cl_len, lane, nl);
    if (lane == 0) {
        uint32_t hclen = kDfCL;
        while (hclen > 4 && !P->cl_len[df_cl_order(hclen - 1)]) hclen--;
        P->hclen = (uint16_t)hclen;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen + (last ? 0 : 3 + 32);
        for (uint32_t s = 0; s < kDfCL; s++) bits += W->freq_cl[s] * (P->cl_len[s] + df_cl_ebits(s));
        for (uint32_t s = 0; s < kDfLL; s++) bits += W->freq_ll[o][s] * (W->len_ll[o][s] + df_ll_ebits(s));
        for (uint32_t s = 0; s < kDfD; s++) bits += W->freq_d[o][s] * (W->len_d[o][s] + df_d_ebits(s));
        P->bits = bits;
    }
    DF_SYNC();
}

// The whole coder for one chunk: src[0, n) -> dst (room for kDfSlot bytes), *res.  tokens: room
// for kDfChunk words (device: global memory, the workgroup's own).  last: the stream's last chunk.
DF_HD void df_code_chunk(DfWork *W, const uint8_t *src, uint32_t n, bool last, uint32_t *tokens, uint8_t *dst,
                         DfResult *res, uint32_t lane, uint32_t nl) {
    if (n == 0) {  // the one chunk of an empty stream: an empty final stored block
        if (lane == 0) {
            dst[0] = 1, dst[1] = 0, dst[2] = 0, dst[3] = 0xFF, dst[4] = 0xFF;
            res->size = 5, res->crc = 0, res->choice = 1, res->n_tok = 0;
        }
        return;
    }
    // ---- stage the chunk, clear the tables
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        struct V16 {
            uint32_t x[4];
        };
        const V16 *s16 = reinterpret_cast<const V16 *>(src);
        V16 *d16 = reinterpret_cast<V16 *>(W->data);
        for (uint32_t i = lane; i < n / 16; i += nl) d16[i] = s16[i];
        for (uint32_t i = (n & ~15u) + lane; i < n; i += nl) W->data[i] = src[i];
    } else {
        for (uint32_t i = lane; i < n; i += nl) W->data[i] = src[i];
    }
    for (uint32_t i = lane; i < (1u << kDfHashBits); i += nl) W->u.head[i] = 0;
    for (uint32_t i = lane; i < 288; i += nl) W->freq_ll[0][i] = W->freq_ll[1][i] = 0;
    for (uint32_t i = lane; i < 32; i += nl) W->freq_d[0][i] = W->freq_d[1][i] = 0;
    for (uint32_t i = lane; i < 256; i += nl) W->crc_tab[i] = df_crc_entry(i);
    if (lane == 0) W->step_any[0] = W->step_any[1] = 0;
    DF_SYNC();
    const uint8_t *d = W->data;
    // ---- CRC-32: a piece per lane, joined by lane 0; literal frequencies of encoding 2
    const uint32_t piece = (n + nl - 1) / nl;
    {
        const uint32_t a = lane * piece < n ? lane * piece : n, b = a + piece < n ? a + piece : n;
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = a; i < b; i++) c = W->crc_tab[(c ^ d[i]) & 0xFF] ^ (c >> 8);
        if (lane < kDfStep) W->crc_part[lane] = ~c;
    }
    for (uint32_t i = lane; i < n; i += nl) DF_ADD(&W->freq_ll[1][d[i]], 1u);
    DF_SYNC();
    if (lane == 0) {
        uint32_t crc = W->crc_part[0];
        const uint32_t xp = df_gf_xpow8(piece);
        for (uint32_t l = 1; l < nl && l * piece < n; l++) {
            const uint32_t len = n - l * piece < piece ? n - l * piece : piece;
            crc = df_crc_join(crc, W->crc_part[l], len == piece ? xp : df_gf_xpow8(len));
        }
        res->crc = crc;
        W->freq_ll[0][256] = W->freq_ll[1][256] = 1;  // end of block
    }
    // ---- matching: tokens, frequencies of encoding 3
    uint32_t ntok = 0, cursor = 0, nmatch = 0;
    for (uint32_t s = 0; s < n; s += kDfStep) {
        uint32_t *any = &W->step_any[(s / kDfStep) & 1];
        for (uint32_t l = lane; l < kDfStep; l += nl) {
            const uint32_t p = s + l;
            uint32_t len = 0, dist = 0;
            if (p >= cursor && p + kDfMinMatch <= n) {
                const uint32_t c = W->u.head[df_hash(d + p)];
                if (c) {
                    const uint32_t m = df_match_len(d, c - 1, p, n);
                    if (m >= kDfMinMatch && !(m == kDfMinMatch && p - (c - 1) > kDfTooFar)) len = m, dist = p - (c - 1);
                }
            }
            W->step_len[l] = (uint16_t)len;
            W->step_dist[l] = (uint16_t)(dist - 1);
            if (len) DF_OR(any, 1u);
        }
        DF_SYNC();
        if (lane == 0) W->step_any[((s / kDfStep) & 1) ^ 1] = 0;
        for (uint32_t l = lane; l < kDfStep; l += nl) {
            const uint32_t p = s + l;
            if (p + kDfMinMatch <= n) DF_MAX(&W->u.head[df_hash(d + p)], p + 1);
        }
        const uint32_t e = s + kDfStep < n ? s + kDfStep : n;
        if (!*any) {  // literals all the way
            if (cursor < e) {
                for (uint32_t p = cursor + lane; p < e; p += nl) {
                    tokens[ntok + (p - cursor)] = d[p];
                    DF_ADD(&W->freq_ll[0][d[p]], 1u);
                }
                ntok += e - cursor;
                cursor = e;
            }
        } else {
            while (cursor < e) {
                const uint32_t i = cursor - s, len = W->step_len[i];
                const bool mine = ntok % nl == lane;
                if (len) {
                    if (mine) {
                        const uint32_t dm1 = W->step_dist[i];
                        uint32_t eb, ex;
                        tokens[ntok] = kDfTokMatch | dm1 << 8 | (len - 3);
                        DF_ADD(&W->freq_ll[0][df_len_sym(len, &eb, &ex)], 1u);
                        DF_ADD(&W->freq_d[0][df_dist_sym(dm1 + 1, &eb, &ex)], 1u);
                    }
                    nmatch++;
                    cursor += len;
                } else {
                    if (mine) {
                        tokens[ntok] = d[cursor];
                        DF_ADD(&W->freq_ll[0][d[cursor]], 1u);
                    }
                    cursor++;
                }
                ntok++;
            }
        }
        DF_SYNC();
    }
    DF_SYNC();
    // ---- cost the three encodings
    df_plan(W, 1, last, lane, nl);
    if (nmatch) df_plan(W, 0, last, lane, nl);  // without a match encoding 3 is encoding 2
    const uint32_t bits1 = 8 * (n + 5), bits2 = W->plan[1].bits, bits3 = nmatch ? W->plan[0].bits : bits2;
    uint32_t choice = 1, best = bits1;
    if (bits2 < best) choice = 2, best = bits2;
    if (bits3 < best) choice = 3, best = bits3;
    if (choice == 1) {
        if (lane == 0) {
            dst[0] = last ? 1 : 0, dst[1] = (uint8_t)n, dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)~n, dst[4] = (uint8_t)(~n >> 8);
            res->size = n + 5, res->choice = 1, res->n_tok = ntok;
        }
        for (uint32_t i = lane; i < n; i += nl) dst[5 + i] = d[i];
        return;
    }
    // ---- write encoding 2 or 3
    const uint32_t o = choice == 3 ? 0 : 1;
    const DfPlan *P = &W->plan[o];
    for (uint32_t i = lane; i < kDfChunk / 4 + 8; i += nl) W->u.out[i] = 0;  // (the position table is done with)
    df_assign_codes(W, W->len_ll[o], kDfLL, 15, W->code_ll, lane, nl);
    df_assign_codes(W, W->len_d[o], kDfD, 15, W->code_d, lane, nl);
    df_assign_codes(W, P->cl_len, kDfCL, 7, W->code_cl, lane, nl);
    uint32_t *out = W->u.out;
    if (lane == 0) {
        uint32_t bp = 0;
        df_put(out, bp, (last ? 1u : 0u) | 2u << 1, 3), bp += 3;
        df_put(out, bp, P->hlit - 257u, 5), bp += 5;
        df_put(out, bp, P->hdist - 1u, 5), bp += 5;
        df_put(out, bp, P->hclen - 4u, 4), bp += 4;
        for (uint32_t i = 0; i < P->hclen; i++) df_put(out, bp, P->cl_len[df_cl_order(i)], 3), bp += 3;
        for (uint32_t i = 0; i < P->n_rle; i++) {
            const uint32_t s = P->rle_sym[i], cl = P->cl_len[s], eb = df_cl_ebits(s);
            df_put(out, bp, W->code_cl[s] | (uint64_t)P->rle_extra[i] << cl, cl + eb), bp += cl + eb;
        }
        W->sc[0] = bp;
    }
    DF_SYNC();
    uint32_t bitpos = W->sc[0];
    const uint32_t nt = o ? n : ntok;
    const uint8_t *ll = W->len_ll[o], *dl = W->len_d[o];
    for (uint32_t b = 0; b < nt; b += kDfStep) {
        for (uint32_t l = lane; l < kDfStep; l += nl) {
            uint32_t nb = 0;
            if (b + l < nt) {
                const uint32_t t = o ? d[b + l] : tokens[b + l];
                if (t & kDfTokMatch) {
                    uint32_t eb, ex;
                    nb = ll[df_len_sym((t & 0xFF) + 3, &eb, &ex)] + eb;
                    nb += dl[df_dist_sym(((t >> 8) & 0x7FFF) + 1, &eb, &ex)] + eb;
                } else
                    nb = ll[t];
            }
            W->step_off[l] = nb;
        }
        DF_SYNC();
        if (lane == 0) {
            uint32_t acc = bitpos;
            for (uint32_t l = 0; l < kDfStep; l++) {
                const uint32_t nb = W->step_off[l];
                W->step_off[l] = acc;
                acc += nb;
            }
            W->step_off[kDfStep] = acc;
        }
        DF_SYNC();
        for (uint32_t l = lane; l < kDfStep; l += nl) {
            if (b + l >= nt) continue;
            const uint32_t t = o ? d[b + l] : tokens[b + l];
            uint64_t v;
            uint32_t nb;
            if (t & kDfTokMatch) {
                uint32_t eb, ex;
                const uint32_t ls = df_len_sym((t & 0xFF) + 3, &eb, &ex);
                v = W->code_ll[ls] | (uint64_t)ex << ll[ls];
                nb = ll[ls] + eb;
                const uint32_t ds = df_dist_sym(((t >> 8) & 0x7FFF) + 1, &eb, &ex);
                v |= ((uint64_t)W->code_d[ds] | (uint64_t)ex << dl[ds]) << nb;
                nb += dl[ds] + eb;
            } else {
                v = W->code_ll[t];
                nb = ll[t];
            }
            df_put(out, W->step_off[l], v, nb);
        }
        bitpos = W->step_off[kDfStep];
        DF_SYNC();
    }
    if (lane == 0) {
        df_put(out, bitpos, W->code_ll[256], ll[256]), bitpos += ll[256];
        uint32_t bytes;
        if (last) {
            bytes = (bitpos + 7) / 8;
        } else {  // an empty stored block: 000, padding, LEN = 0, NLEN = ffff
            bytes = (bitpos + 3 + 7) / 8;
            df_put(out, bytes * 8 + 16, 0xFFFFu, 16);
            bytes += 4;
        }
        W->sc[1] = bytes;
        res->size = bytes, res->choice = choice, res->n_tok = ntok;
    }
    DF_SYNC();
    const uint32_t bytes = W->sc[1];
    for (uint32_t i = lane; i < bytes; i += nl) dst[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
}

// the 10 header bytes of a member (block_codec.cpp's gzip_append writes the same)
DF_HD uint8_t df_gzip_header(uint32_t i) { return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 9 ? 0xff : 0; }

// Host restatement: the member of data[0, n) into out (room for df_member_bound(n) bytes);
// returns its size.  choices, if given, receives each chunk's encoding (df_chunks(n) bytes).
inline uint64_t df_member_host(const uint8_t *data, uint64_t n, uint8_t *out, uint8_t *choices = nullptr) {
    DfWork *W = new DfWork;
    uint32_t *tokens = new uint32_t[kDfChunk];
    uint8_t *slot = new uint8_t[kDfSlot];
    for (uint32_t i = 0; i < 10; i++) out[i] = df_gzip_header(i);
    uint64_t at = 10;
    uint32_t crc = 0;
    const uint64_t nc = df_chunks(n);
    for (uint64_t c = 0; c < nc; c++) {
        const uint64_t off = c * kDfChunk;
        const uint32_t m = (uint32_t)(n - off < kDfChunk ? n - off : kDfChunk);
        DfResult r{};
        df_code_chunk(W, data + off, m, c + 1 == nc, tokens, slot, &r, 0, 1);
        std::memcpy(out + at, slot, r.size);
        at += r.size;
        crc = c ? df_crc_join(crc, r.crc, df_gf_xpow8(m)) : r.crc;
        if (choices) choices[c] = (uint8_t)r.choice;
    }
    const uint32_t isize = (uint32_t)n;
    for (int i = 0; i < 4; i++) out[at++] = (uint8_t)(crc >> (8 * i));
    for (int i = 0; i < 4; i++) out[at++] = (uint8_t)(isize >> (8 * i));
    delete[] slot;
    delete[] tokens;
    delete W;
    return at;
}

}  // namespace ntc
