// FASTQ quality scores: the per-byte and per-word logic of the kernels in quality.hip.
// Written once as host + device code, like nonacgt_core.h: the HIP kernels call these
// functions, and a CPU program (tests/quality_cpu) compiles the very same functions with a
// host compiler, so the table / alphabet / pack / unpack logic is checked without a GPU.
//
// Vocabulary (DESIGN.md "Quality scores"): a block's qualities are the quality bytes of its
// reads, read by read.  Its presence map has bit c set when byte c occurs; only '!'..'~'
// (33..126) can occur, so two 64-bit words hold it: p0 = bits 0..63, p1 = bits 64..127.  The
// alphabet is the set bits in ascending order, a byte's code its rank among them, and a code
// takes w = q_width(n_syms) bits of a little-endian stream of 64-bit words.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Q_HD __host__ __device__ __forceinline__
#else
#define Q_HD inline
#endif

namespace ntc {

constexpr uint32_t kQDrop = 0, kQKeep = 1, kQBin8 = 2;  // the "qualities" option
constexpr uint32_t kQLo = 33, kQHi = 126;               // '!' .. '~'

Q_HD uint32_t q_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}

// Phred q -> the 8-level scale's representative (q < 2 stays: '!' and '"' mean "no call")
Q_HD uint32_t q_bin8(uint32_t q) {
    if (q < 2) return q;
    if (q < 10) return 6;
    if (q < 20) return 15;
    if (q < 25) return 22;
    if (q < 30) return 27;
    if (q < 35) return 33;
    if (q < 40) return 37;
    return 40;
}

// entry c of a mode's 256-entry table: the byte kept for input byte c, 0 = not a quality
Q_HD uint32_t q_table(uint32_t mode, uint32_t c) {
    if (c < kQLo || c > kQHi) return 0;
    return mode == kQBin8 ? kQLo + q_bin8(c - kQLo) : c;
}

// bits per code for an alphabet of n symbols: powers of two, so no code straddles a byte
Q_HD uint32_t q_width(uint32_t n) { return n <= 1 ? 0 : n == 2 ? 1 : n <= 4 ? 2 : n <= 16 ? 4 : 8; }

Q_HD uint32_t q_nsyms(uint64_t p0, uint64_t p1) { return q_popc(p0) + q_popc(p1); }

// the code of byte c (< 128): set bits below c
Q_HD uint32_t q_rank(uint64_t p0, uint64_t p1, uint32_t c) {
    return c < 64 ? q_popc(p0 & ((1ull << c) - 1)) : q_popc(p0) + q_popc(p1 & ((1ull << (c - 64)) - 1));
}

// alphabet[0 .. n_syms): the set bits, ascending; returns n_syms (<= 94 for maps made from
// q_table bytes, <= 96 entries are written whatever the map holds)
Q_HD uint32_t q_alphabet(uint64_t p0, uint64_t p1, uint8_t *alphabet) {
    uint32_t n = 0;
    for (uint32_t c = 0; c < 128 && n < 96; c++)
        if (((c < 64 ? p0 : p1) >> (c & 63)) & 1) alphabet[n++] = (uint8_t)c;
    return n;
}

// 64-bit words of n codes of w bits
Q_HD uint64_t q_words(uint64_t n, uint32_t w) { return (n * w + 63) / 64; }

// Eight quality bytes (v, little-endian; the first `live` count, the rest are past the
// block's end) -> their 8 w code bits, first byte lowest.  w > 0.
Q_HD uint64_t q_pack8(uint64_t v, uint32_t live, uint64_t p0, uint64_t p1, uint32_t w) {
    uint64_t out = 0;
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t c = (uint32_t)(v >> (8 * j)) & 0x7F;
        const uint64_t code = j < live ? q_rank(p0, p1, c) : 0;
        out |= code << (j * w);
    }
    return out;
}

// code i of a packed stream (w > 0)
Q_HD uint32_t q_code_at(const uint64_t *words, uint64_t i, uint32_t w) {
    const uint64_t bit = i * w;
    return (uint32_t)(words[bit >> 6] >> (bit & 63)) & ((1u << w) - 1);
}

// A section's header fields as a decoder may trust them: the width follows from n_syms, the
// alphabet ascends inside '!'..'~', and an empty block has no symbols.
Q_HD bool q_meta_ok(uint64_t n_quals, uint32_t width, uint32_t n_syms, const uint8_t *alphabet) {
    if (n_syms > 94 || width != q_width(n_syms) || (n_quals == 0) != (n_syms == 0)) return false;
    for (uint32_t i = 0; i < n_syms; i++) {
        if (alphabet[i] < kQLo || alphabet[i] > kQHi) return false;
        if (i && alphabet[i] <= alphabet[i - 1]) return false;
    }
    return true;
}

}  // namespace ntc
