// Per-block content digests on the GPU (digest_core.h has the arithmetic, DESIGN.md "Content
// digests").  One streaming pass over bytes that are in HBM anyway:
//   k_dg_init     encode: the block table (reads, bases, components), digests zeroed
//   k_dg_sum      a workgroup per kDgChunk consecutive strings, block after block of those it
//                 touches.  A quarter-wave per string up to kDgLong bytes: the lanes take its
//                 64-bit words 16 at a time, each from two aligned loads and a funnel shift,
//                 the inner sum closes in the quarter-wave, its lane 0 adds the string's outer
//                 term.  Longer strings are listed in LDS and then taken one by one by the
//                 whole workgroup.  The terms are summed over the workgroup; one lane issues
//                 one 64-bit atomic per block touched.
//   k_dg_compare  decode: one workgroup over the blocks, the computed words against the expected;
//                 the first read of a block that differs goes to the decode status.
// Every position is clamped to the buffer: offsets a damaged input produced cost a wrong
// digest (and so a mismatch), never an access outside it.
#include <hip/hip_runtime.h>

#include "digest_core.h"
#include "kernels.h"

namespace ntc {

namespace {

constexpr uint32_t kDgChunk = 1024;  // strings per workgroup
static_assert(kDgChunk % 16 == 0, "a workgroup's quarter-waves step through its chunk");

__device__ __forceinline__ uint64_t umin(uint64_t x, uint64_t y) { return x < y ? x : y; }

struct DgSpan {
    uint64_t p, n;  // first byte in buf (bias included), bytes; inside [0, bias + buf_bytes)
};
__device__ __forceinline__ DgSpan dg_span(const DigestArgs &a, uint64_t r) {
    uint64_t p, n;
    if (a.offs) {
        const uint64_t o0 = a.origin ? *a.origin : 0, b = a.offs[r], e = a.offs[r + 1];
        p = b - o0;
        n = e - b;
        if (b < o0 || e < b) p = n = 0;  // (offsets out of order: a failed walk)
    } else {
        p = a.start[r];
        n = a.len[r];
    }
    DgSpan s;
    s.p = umin(p, a.buf_bytes);
    s.n = umin(n, a.buf_bytes - s.p);
    s.p += a.bias;
    return s;
}

// word j of the string at s (j < dg_words(s.n)): aligned loads only, none past the aligned
// word that holds the string's last byte
__device__ __forceinline__ uint64_t dg_load(const uint64_t *q, const DgSpan &s, uint64_t j) {
    const uint32_t mis = (uint32_t)(s.p & 7);
    const uint64_t at = (s.p >> 3) + j;
    const uint64_t lo = q[at];
    const uint64_t hi = dg_needs_hi(s.n, j, mis) ? q[at + 1] : 0;
    return dg_funnel(lo, hi, 8 * mis) & dg_tail_mask(s.n, j);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int d = 32; d; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}

// the sum of v over the workgroup, valid in thread 0; red: 4 words of LDS, free to reuse
// after the barrier that follows the caller's use of the result
__device__ __forceinline__ uint64_t group_sum(uint64_t v, uint64_t *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void k_dg_init(DigestMetaDev *t, uint64_t n_blocks, uint64_t n_reads,
                                                 uint32_t block_reads, const uint64_t *offs, uint32_t components,
                                                 uint32_t keep) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const uint64_t r0 = b * block_reads, r1 = umin(r0 + block_reads, n_reads);
    DigestMetaDev &m = t[b];
    m.n_reads = r1 - r0;
    m.n_bases = offs[r1] - offs[r0];
    for (uint32_t c = 0; c < 4; c++)
        if (!(keep >> c & 1)) m.d[c] = 0;
    m.components = components;
    m.pad = 0;
}

__global__ __launch_bounds__(256) void k_dg_sum(DigestArgs a) {
    __shared__ uint32_t long_list[kDgChunk];
    __shared__ uint32_t n_long;
    __shared__ uint64_t red[4];
    if (a.status && *a.status != ~0ull) return;  // a failed call: its offsets are not to be trusted
    const uint32_t tid = threadIdx.x, ql = tid & 15, quarter = tid >> 4;
    const uint64_t c0 = (uint64_t)blockIdx.x * kDgChunk, c1 = umin(c0 + kDgChunk, a.n_reads);
    const uint64_t *q = (const uint64_t *)a.buf;
    for (uint64_t lo = c0; lo < c1;) {
        const uint64_t b = lo / a.block_reads, hi = umin(c1, (b + 1) * a.block_reads), i0 = lo - b * a.block_reads;
        if (tid == 0) n_long = 0;
        __syncthreads();
        uint64_t acc = 0;  // outer terms: lane 0 of each quarter-wave, and thread 0 for the long strings
        for (uint64_t r = lo + quarter; r < hi; r += 16) {
            const DgSpan s = dg_span(a, r);
            if (s.n > kDgLong) {
                if (ql == 0) long_list[atomicAdd(&n_long, 1u)] = (uint32_t)(r - lo);
                continue;
            }
            const uint64_t words = dg_words(s.n);
            uint64_t inner = 0;
            for (uint64_t j = ql; j < words; j += 16) inner += dg_word_term(dg_load(q, s, j), j);
            for (int d = 8; d; d >>= 1) inner += (uint64_t)__shfl_xor((unsigned long long)inner, d);
            if (ql == 0) acc += dg_read_term(dg_string(s.n, inner), i0 + (r - lo));
        }
        __syncthreads();
        const uint32_t nl = n_long;
        for (uint32_t t = 0; t < nl; t++) {
            const uint64_t r = lo + long_list[t];
            const DgSpan s = dg_span(a, r);
            const uint64_t words = dg_words(s.n);
            uint64_t inner = 0;
            for (uint64_t j = tid; j < words; j += 256) inner += dg_word_term(dg_load(q, s, j), j);
            inner = group_sum(inner, red);
            if (tid == 0) acc += dg_read_term(dg_string(s.n, inner), i0 + (r - lo));
            __syncthreads();
        }
        const uint64_t sum = group_sum(acc, red);
        if (tid == 0) atomicAdd((unsigned long long *)(a.out + b * a.out_stride), (unsigned long long)sum);
        __syncthreads();
        lo = hi;
    }
}

// One workgroup: the call has few blocks, and every thread has read the status before any
// sets it, so the verdict does not depend on the order the blocks are looked at.
__global__ __launch_bounds__(256) void k_dg_compare(DigestCmpArgs a) {
    const bool failed = *a.status != ~0ull;  // the call failed already: that verdict stands
    __syncthreads();
    if (failed) return;
    for (uint64_t b = threadIdx.x; b < a.n_blocks; b += 256) {
        const DigestMetaDev &e = a.expected[b];
        DigestMetaDev &g = a.computed[b];
        const uint64_t r0 = a.r0[b], r1 = a.r0[b + 1];
        g.n_bases = r1 <= a.n_reads && r0 <= r1 ? a.offs[r1] - a.offs[r0] : 0;
        const uint32_t check = e.components & a.checkable;
        bool bad = g.n_bases != e.n_bases;
        for (uint32_t c = 0; c < 4; c++) bad |= (check >> c & 1) && g.d[c] != e.d[c];
        if (bad) atomicMin(a.status, (unsigned long long)(r0 << 8 | kErrDigest));
    }
}

}  // namespace

void launch_digest_init(DigestMetaDev *table, uint64_t n_blocks, uint64_t n_reads, uint32_t block_reads,
                        const uint64_t *offs, uint32_t components, uint32_t keep, hipStream_t s) {
    if (n_blocks == 0) return;
    hipLaunchKernelGGL(k_dg_init, dim3((uint32_t)((n_blocks + 255) / 256)), dim3(256), 0, s, table, n_blocks, n_reads,
                       block_reads, offs, components, keep);
}

void launch_digest(const DigestArgs &args, hipStream_t s) {
    if (args.n_reads == 0 || args.block_reads == 0) return;
    DigestArgs a = args;
    // the kernel loads aligned 64-bit words: an unaligned buffer starts bias bytes into one
    a.bias = (uint32_t)((uintptr_t)a.buf & 7);
    a.buf -= a.bias;
    hipLaunchKernelGGL(k_dg_sum, dim3((uint32_t)((a.n_reads + kDgChunk - 1) / kDgChunk)), dim3(256), 0, s, a);
}

void launch_digest_compare(const DigestCmpArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    hipLaunchKernelGGL(k_dg_compare, dim3(1), dim3(256), 0, s, a);
}

}  // namespace ntc
