// Per-block content digests: the arithmetic of the kernels in digest.hip.  Written once as
// host + device code, like names_core.h and qrans_core.h: the HIP kernels call these
// functions, and a CPU program (tests/digest_cpu) compiles the very same functions with a
// host compiler, so the definition is checked without a GPU.
//
// Definition (DESIGN.md "Content digests"; all arithmetic mod 2^64).  For a byte string s of
// n bytes, w_j = the little-endian 64-bit word of s[8j .. 8j + 8), zero-padded past n:
//   h(s) = mix((n + 1) K0 + sum_j mix(w_j + (j + 1) K1))
// and for the strings s_0 .. s_{m-1} of a block, i = the index inside the block:
//   D    = sum_i mix(h(s_i) + (i + 1) K1)
// Both sums are plain integer sums, so any split of words over lanes and of reads over
// waves, workgroups and atomics gives the same bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DG_HD __host__ __device__ __forceinline__
#else
#define DG_HD inline
#endif

namespace ntc {

constexpr uint64_t kDgK0 = 0xD6E8FEB86659FD93ull, kDgK1 = 0x9E3779B97F4A7C15ull;
// component bits of ntc_digest_meta.components, and their order in its d_* words
constexpr uint32_t kDgSeq = 1, kDgSym = 2, kDgQual = 4, kDgName = 8, kDgAll = 15;
constexpr int kErrDigest = 12;  // NTC_ERR_DIGEST, a decode status code beside encode_core.h's

// a section's meta on its own (ntc_digest_meta: components, reserved, d = d_seq .. d_name):
// known bits, seq among them, nothing set for an absent component
DG_HD bool dg_meta_ok(uint32_t components, uint32_t reserved, const uint64_t d[4]) {
    if ((components & ~kDgAll) || !(components & kDgSeq) || reserved) return false;
    for (uint32_t c = 0; c < 4; c++)
        if (!(components >> c & 1) && d[c]) return false;
    return true;
}

DG_HD uint64_t dg_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// what word j of a string adds to the string's inner sum
DG_HD uint64_t dg_word_term(uint64_t w, uint64_t j) { return dg_mix(w + (j + 1) * kDgK1); }
// h of a string of n bytes from its complete inner sum
DG_HD uint64_t dg_string(uint64_t n, uint64_t inner) { return dg_mix((n + 1) * kDgK0 + inner); }
// what string i of a block adds to the block's digest
DG_HD uint64_t dg_read_term(uint64_t h, uint64_t i) { return dg_mix(h + (i + 1) * kDgK1); }

// words of a string of n bytes
DG_HD uint64_t dg_words(uint64_t n) { return (n + 7) / 8; }
// the bytes of word j that belong to a string of n bytes (j < dg_words(n)): the others are zero
DG_HD uint64_t dg_tail_mask(uint64_t n, uint64_t j) {
    const uint64_t left = n - 8 * j;
    return left >= 8 ? ~0ull : (1ull << (8 * left)) - 1;
}
// word j of the string that starts sh / 8 bytes into the aligned word lo (hi: the aligned
// word after it, needed only when dg_needs_hi)
DG_HD uint64_t dg_funnel(uint64_t lo, uint64_t hi, uint32_t sh) { return sh ? lo >> sh | hi << (64 - sh) : lo; }
// word j of a string of n bytes that starts mis bytes (0..7) into an aligned word takes bytes
// from the following aligned word too
DG_HD bool dg_needs_hi(uint64_t n, uint64_t j, uint32_t mis) { return mis && n - 8 * j > 8 - mis; }

}  // namespace ntc
