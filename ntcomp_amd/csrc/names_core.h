// FASTQ read names: the per-name logic of the kernels in names.hip.  Written once as host +
// device code, like quality_core.h: the HIP kernels call these functions, and a CPU program
// (tests/names_cpu) compiles the very same functions with a host compiler and walks them in
// the kernels' 64-byte steps, so the cut / prefix / suffix / section logic is checked
// without a GPU.
//
// Vocabulary (DESIGN.md "Read names"): a read's name is its header line without the '@' and
// without one trailing '\r'; under mode id it ends before its first space or tab.  Inside a
// block of block_reads reads the chain restarts every kNGroup reads; read i of a group has
// pre = bytes shared with the head of its predecessor, suf = bytes shared with its tail (both
// capped at 255 and never overlapping in either name), mid = what lies between.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define N_HD __host__ __device__ __forceinline__
#else
#define N_HD inline
#endif

namespace ntc {

constexpr uint32_t kNDrop = 0, kNKeep = 1, kNId = 2;  // the "names" option
constexpr uint32_t kNMax = 4095;                      // NTC_NAME_MAX
constexpr uint32_t kNGroup = 64;                      // NTC_NAME_GROUP
constexpr uint32_t kNCap = 255;                       // pre and suf are one byte each

N_HD uint32_t n_ctz(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)x) - 1;
#else
    return (uint32_t)__builtin_ctzll(x);
#endif
}

// mode id cuts the name before this byte
N_HD bool n_is_cut(uint32_t c) { return c == ' ' || c == '\t'; }

// One 64-byte step of a comparison: bit j of eq says that lane j's bytes agree, live lanes
// take part (1..64); the lanes that agree before the first that does not.
N_HD uint32_t n_run(uint64_t eq, uint32_t live) {
    const uint64_t m = live >= 64 ? ~0ull : (1ull << live) - 1;
    const uint64_t ne = ~eq & m;
    return ne ? n_ctz(ne) : live;
}

// how far the prefix comparison may go, and the suffix comparison once pre is known
N_HD uint32_t n_pre_limit(uint32_t plen, uint32_t len) {
    const uint32_t m = plen < len ? plen : len;
    return m < kNCap ? m : kNCap;
}
N_HD uint32_t n_suf_limit(uint32_t plen, uint32_t len, uint32_t pre) {
    const uint32_t m = (plen < len ? plen : len) - pre;  // pre <= both
    return m < kNCap ? m : kNCap;
}

// the decode side's per-read conditions: i = the read's index inside its block
N_HD bool n_read_ok(uint32_t i, uint32_t len, uint32_t pre, uint32_t suf, uint32_t plen) {
    if (len > kNMax) return false;
    if (i % kNGroup == 0) return pre == 0 && suf == 0;
    return pre + suf <= len && pre + suf <= plen;
}

// byte j of a name from its predecessor (p, plen) and its mid; valid for a read n_read_ok took
N_HD uint8_t n_byte(const uint8_t *p, uint32_t plen, const uint8_t *mid, uint32_t len, uint32_t pre, uint32_t suf,
                    uint32_t j) {
    if (j < pre) return p[j];
    if (j < len - suf) return mid[j - pre];
    return p[plen - (len - j)];
}

// bytes of a section's payload: the three columns (4 n), the mids, zeros to a multiple of 8
N_HD uint64_t n_payload_bytes(uint64_t n_reads, uint64_t mid_bytes) { return (4 * n_reads + mid_bytes + 7) / 8 * 8; }

// the counts of a section's meta (ntc_name_meta) agree with one another (payload_off is the caller's)
N_HD bool n_meta_ok(uint64_t n_reads, uint64_t name_bytes, uint64_t mid_bytes, uint64_t payload_bytes) {
    return !(n_reads >> 40) && mid_bytes <= name_bytes && name_bytes <= n_reads * kNMax &&
           payload_bytes == n_payload_bytes(n_reads, mid_bytes);
}

}  // namespace ntc
