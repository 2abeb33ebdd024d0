// Non-ACGT symbols (N and the IUPAC codes): the per-chunk, per-read and per-run logic of the
// kernels in nonacgt.hip.  Written once as host + device code, like encode_core.h: the HIP
// kernels call these functions, and a CPU program (tests/nonacgt_cpu) compiles the very same
// functions with a host compiler, so the flag / mark / emit logic is checked without a GPU.
//
// Vocabulary (DESIGN.md "Non-ACGT symbols"): positions are batch positions, 0 = the first
// base of the call's first read.  A chunk is 16 consecutive positions, a word 64 (four
// chunks; bit x % 64 of word x / 64).  Three bitmaps of one bit per position:
//   M  the byte is not A/C/G/T                      (flag pass)
//   S  a run starts here: M, and the previous byte differs or the position starts a read
//   E  a run ends here:   M, and the next byte differs or the position ends a read
// The flag pass sets the S / E bits that neighbouring bytes decide; the per-read pass adds
// the bits at read boundaries.  S and E hold equally many bits, and the i-th start pairs
// with the i-th end: no thread ever walks a run.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NX_HD __host__ __device__ __forceinline__
#else
#define NX_HD inline
#endif

namespace ntc {

// ntc_nx_run (include/ntcomp_gpu.h), 24 bytes
struct NxRun {
    uint64_t read;
    uint32_t pos, len, sym, reserved;
};

constexpr uint32_t kNxNone = 0x100u;  // "no neighbour": the batch's first / last position

NX_HD bool nx_is_base(uint32_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
// the twelve symbols normalize(true) keeps beside A/C/G/T (fastx.cpp, fastq.hip)
NX_HD bool nx_is_symbol(uint32_t b) {
    switch (b) {
    case 'N': case '-': case 'B': case 'D': case 'H': case 'V':
    case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M': return true;
    default: return false;
    }
}

// bit j = byte j of d is non-zero
NX_HD uint32_t nx_nonzero4(uint32_t d) {
    const uint32_t y = ((d | ((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7) & 0x01010101u;
    return (y * 0x10204080u) >> 28;  // bits 0, 8, 16, 24 -> 0..3 (no two products meet)
}
// bit j = byte j of w is not one of A/C/G/T: k_pack's round trip, code -> "ACGT"[code]
NX_HD uint32_t nx_bad4(uint32_t w) {
    const uint32_t t = ((w >> 1) ^ (w >> 2)) & 0x03030303u;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t back = __builtin_amdgcn_perm(0u, 0x54474341u, t);
#else
    uint32_t back = 0;
    for (int j = 0; j < 4; j++) back |= ((0x54474341u >> (8 * ((t >> (8 * j)) & 3u))) & 0xFFu) << (8 * j);
#endif
    return nx_nonzero4(back ^ w);
}

struct NxFlags {
    uint32_t m, s, e;  // 16 bits each, bit j = chunk position j
};
// One chunk: w = its 16 bytes (little-endian words), n = how many lie inside the batch
// (1..16; the bytes past n are ignored), prev / next = the bytes on either side or kNxNone
// at the batch's ends (next is only read when n = 16).  Read boundaries are not known here.
NX_HD NxFlags nx_chunk_flags(const uint32_t w[4], uint32_t n, uint32_t prev, uint32_t next) {
    NxFlags f;
    const uint32_t valid = n >= 16 ? 0xFFFFu : ((1u << n) - 1u);
    f.m = (nx_bad4(w[0]) | nx_bad4(w[1]) << 4 | nx_bad4(w[2]) << 8 | nx_bad4(w[3]) << 12) & valid;
    f.s = f.e = 0;
    if (!f.m) return f;
    // dp bit j: byte j differs from byte j - 1
    uint32_t dp = nx_nonzero4(w[0] ^ (w[0] << 8 | (prev & 0xFFu))) | nx_nonzero4(w[1] ^ (w[1] << 8 | w[0] >> 24)) << 4 |
                  nx_nonzero4(w[2] ^ (w[2] << 8 | w[1] >> 24)) << 8 | nx_nonzero4(w[3] ^ (w[3] << 8 | w[2] >> 24)) << 12;
    if (prev > 0xFFu) dp |= 1u;
    // dn bit j: byte j differs from byte j + 1; the last valid byte asks `next`
    const uint32_t last = n >= 16 ? 15u : n - 1u;
    const uint32_t nd = (n < 16 || next > 0xFFu || next != (w[3] >> 24)) ? 1u : 0u;
    const uint32_t dn = ((dp >> 1) & ~(1u << last)) | nd << last;
    f.s = f.m & dp;
    f.e = f.m & dn;
    return f;
}

NX_HD bool nx_bit(const uint64_t *bm, uint64_t x) { return (bm[x >> 6] >> (x & 63)) & 1u; }

// position of the k-th (0-based) set bit of w; w has more than k bits
NX_HD uint32_t nx_select64(uint64_t w, uint32_t k) {
    for (uint32_t j = 0; j < k; j++) w &= w - 1;
    return (uint32_t)__builtin_ctzll(w);
}
// largest i in [0, n) with a[i] <= v (a non-decreasing, a[0] <= v)
NX_HD uint64_t nx_last_le(const uint64_t *a, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// Run i of the batch: the i-th set bit of S and of E (soff / eoff: exclusive prefix counts
// of the words' bits, n_words + 1 entries), its read by one search in offs (n_reads + 1
// absolute offsets; batch position x is byte offs[0] + x of bases).  false: pos or len does
// not fit 32 bits.
NX_HD bool nx_emit_run(uint64_t i, const uint64_t *S, const uint64_t *E, const uint64_t *soff, const uint64_t *eoff,
                       uint64_t n_words, const uint8_t *bases, const uint64_t *offs, uint64_t n_reads, NxRun &out) {
    const uint64_t ws = nx_last_le(soff, n_words + 1, i), we = nx_last_le(eoff, n_words + 1, i);
    const uint64_t a = ws * 64 + nx_select64(S[ws], (uint32_t)(i - soff[ws]));
    const uint64_t b = we * 64 + nx_select64(E[we], (uint32_t)(i - eoff[we]));
    const uint64_t r = nx_last_le(offs, n_reads + 1, offs[0] + a);
    const uint64_t pos = offs[0] + a - offs[r], len = b - a + 1;
    out.read = r;
    out.pos = (uint32_t)pos;
    out.len = (uint32_t)len;
    out.sym = bases[offs[0] + a];
    out.reserved = 0;
    return pos <= 0xFFFFFFFFull && len <= 0xFFFFFFFFull;
}

// decode side: a run (or a piece of one) against the decoded reads' offsets
NX_HD bool nx_run_fits(const NxRun &r, const uint64_t *offs, uint64_t n_reads) {
    if (r.read >= n_reads || r.len == 0 || !nx_is_symbol(r.sym)) return false;
    return (uint64_t)r.pos + r.len <= offs[r.read + 1] - offs[r.read];
}

// the substitute base: the lowest of A, C, G, T the index contains (absent: bit c set = no
// node ends with character c); 0 when it contains none
NX_HD uint32_t nx_substitute(uint32_t absent) {
    for (uint32_t c = 0; c < 4; c++)
        if (!((absent >> c) & 1u)) return (0x54474341u >> (8 * c)) & 0xFFu;
    return 0;
}

}  // namespace ntc
