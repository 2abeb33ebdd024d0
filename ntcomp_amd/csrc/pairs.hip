// Paired-end reads on the GPU (pair_core.h has the logic, DESIGN.md "Paired-end reads").
// Encode, over two FASTQ texts in HBM and their newline tables (fastq.hip launch_fastq_lines):
//   k_pw_sizes   a thread per pair: both texts hold exactly 4 n_pairs lines (else the weave's
//                status word is set and nothing below writes), the bytes of the pair's two
//                records, a newline more where a text's last line lacks its own
//   (scan)       exclusive scan -> each pair's place in the woven text
//   k_pw_copy    one wave per pair, lanes across bytes: record p of text 1, then record p of
//                text 2, into the buffer the FASTQ parse reads
//   k_pm_check   after the parse, over the woven text and its newline table: one wave per pair,
//                the id cut by ballot + ctz, the "/1" "/2" strip, the comparison in 64-byte
//                ballot steps; atomicMin of (2 p) << 8 | NTC_ERR_FORMAT on the pass's own word
//   k_pair_box   both status words to the host mailbox (read at the parse's sync)
// Decode, over the text a formatter wrote and the per-read offsets it left:
//   k_ps_sizes   a thread per pair: the bytes of its even and of its odd read
//   (scan x 2)   -> each read's place inside its part
//   k_ps_copy    one wave per read: all mate-1 records in order, then all mate-2 records; part
//                1's bytes to the mailbox.  A failed call (every size 0) writes nothing.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pair_core.h"
#include "window_core.h"

namespace ntc {

namespace {

struct PText {
    uint64_t n_nl;
    uint32_t last;
    bool ok;
};
__device__ __forceinline__ PText p_text(const PairWeaveArgs &a, int t) {
    PText x;
    x.n_nl = *a.n_nl_p[t];
    x.last = a.n_raw[t] ? a.raw[t][a.n_raw[t] - 1] : 0;
    x.ok = p_text_ok(x.n_nl, a.n_raw[t], x.last, a.n_pairs);
    return x;
}

__global__ __launch_bounds__(256) void k_pw_sizes(PairWeaveArgs a) {
    const PText t0 = p_text(a, 0), t1 = p_text(a, 1);
    if (!t0.ok || !t1.ok) {  // the first read without its record, in the text that is short or long
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const PText &t = t0.ok ? t1 : t0;
            const uint64_t whole = p_lines(t.n_nl, a.n_raw[t0.ok ? 1 : 0], t.last) / 4;
            const uint64_t p = whole < a.n_pairs ? whole : (a.n_pairs ? a.n_pairs - 1 : 0);
            atomicMin(a.status, (unsigned long long)((2 * p + (t0.ok ? 1 : 0)) << 8 | kErrFormat));
        }
        return;
    }
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_pairs) return;
    uint64_t sz = p_rec_end(a.nl[0], t0.n_nl, a.n_raw[0], p) - p_rec_begin(a.nl[0], p);
    sz += p_rec_end(a.nl[1], t1.n_nl, a.n_raw[1], p) - p_rec_begin(a.nl[1], p);
    if (p == a.n_pairs - 1) sz += (p_adds_nl(a.n_raw[0], t0.last) ? 1 : 0) + (p_adds_nl(a.n_raw[1], t1.last) ? 1 : 0);
    a.sizes[p] = (uint32_t)sz;  // (both texts together stay under 4 GiB)
}

__global__ __launch_bounds__(256) void k_pw_copy(PairWeaveArgs a) {
    if (*a.status != ~0ull) return;  // a text with another line count: nothing is woven
    if (a.offs[a.n_pairs] != a.out_bytes) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(a.status, (unsigned long long)kErrFormat);
        return;
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    uint64_t n_nl[2];
    bool adds[2];
    for (int t = 0; t < 2; t++) {
        n_nl[t] = *a.n_nl_p[t];
        adds[t] = p_adds_nl(a.n_raw[t], a.n_raw[t] ? a.raw[t][a.n_raw[t] - 1] : 0);
    }
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += waves) {
        uint8_t *dst = a.out + a.offs[p];
        for (int t = 0; t < 2; t++) {
            const uint64_t b = p_rec_begin(a.nl[t], p), len = p_rec_end(a.nl[t], n_nl[t], a.n_raw[t], p) - b;
            const uint8_t *src = a.raw[t] + b;
            for (uint64_t i = lane; i < len; i += 64) dst[i] = src[i];
            dst += len;
            if (p == a.n_pairs - 1 && adds[t]) {
                if (lane == 0) *dst = '\n';
                dst++;
            }
        }
    }
}

struct PName {
    uint64_t s;
    uint32_t len;
};
// id(name of record r) of the woven text (wave-uniform; every lane takes part in the ballots)
__device__ __forceinline__ PName p_id(const PairCheckArgs &a, uint64_t r, uint32_t lane) {
    const uint64_t h0 = r ? (uint64_t)a.nl[4 * r - 1] + 1 : 0, e = a.nl[4 * r];
    PName f;
    f.s = h0 + 1 < e ? h0 + 1 : e;  // (the parse saw '@' at h0)
    uint32_t len = (uint32_t)(e - f.s);
    if (len && a.raw[e - 1] == '\r') len--;
    for (uint32_t b = 0; b < len; b += 64) {
        const uint32_t i = b + lane;
        if (p_cut_step(__ballot(i < len && n_is_cut(a.raw[f.s + i])), b, &len)) break;
    }
    f.len = len;
    return f;
}

__global__ __launch_bounds__(256) void k_pm_check(PairCheckArgs a) {
    if (*a.parse_status != ~0ull) return;  // the text failed the parse: its line table says nothing
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += waves) {
        PName x = p_id(a, 2 * p, lane), y = p_id(a, 2 * p + 1, lane);
        if (p_strips(x.len, y.len, x.len >= 2 ? a.raw[x.s + x.len - 2] : 0, x.len >= 2 ? a.raw[x.s + x.len - 1] : 0,
                     y.len >= 2 ? a.raw[y.s + y.len - 2] : 0, y.len >= 2 ? a.raw[y.s + y.len - 1] : 0)) {
            x.len -= 2;
            y.len -= 2;
        }
        bool agree = x.len == y.len;
        for (uint32_t b = 0; agree && b < x.len; b += 64) {
            const uint32_t i = b + lane;
            agree = p_step_agrees(__ballot(i < x.len && a.raw[x.s + i] == a.raw[y.s + i]), x.len, b);
        }
        if (!agree && lane == 0) atomicMin(a.status, (unsigned long long)((2 * p) << 8 | kErrFormat));
    }
}

__global__ void k_pair_box(const unsigned long long *weave, const unsigned long long *check, uint64_t *box) {
    box[kBoxWeave] = *weave;
    box[kBoxMateCheck] = *check;
}

// ---- decode -----------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ps_sizes(const uint64_t *out_offs, uint64_t n_pairs, uint64_t *s1, uint64_t *s2) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    s1[p] = out_offs[2 * p + 1] - out_offs[2 * p];
    s2[p] = out_offs[2 * p + 2] - out_offs[2 * p + 1];
}

__global__ __launch_bounds__(256) void k_ps_copy(PairSplitArgs a) {
    const uint64_t n = 2 * a.n_pairs;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.box[kBoxPairFirst] = a.o1[a.n_pairs];
    if (a.out_offs[n] == 0 || a.out_offs[n] > a.cap) return;  // a failed call (sizes 0) or a short buffer
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += waves) {
        const uint64_t b = a.out_offs[r], len = a.out_offs[r + 1] - b;
        if (w_skips(b, b + len)) continue;  // a read outside the call's window has no record
        const uint8_t *src = a.text + b;
        uint8_t *dst = a.out + p_split_at(r, a.o1, a.o2, a.n_pairs);
        for (uint64_t i = lane; i < len; i += 64) dst[i] = src[i];
    }
}

}  // namespace

void launch_pair_weave(const PairWeaveArgs &a, hipStream_t s) {
    (void)hipMemsetAsync(a.status, 0xFF, 8, s);
    if (a.n_pairs == 0) return;  // (the caller refused text for zero pairs)
    hipLaunchKernelGGL(k_pw_sizes, dim3((uint32_t)((a.n_pairs + 255) / 256)), dim3(256), 0, s, a);
    scan_excl_u32(a.sizes, a.n_pairs, a.offs, a.tmp, s);
    const uint64_t blocks = std::min<uint64_t>((a.n_pairs + 3) / 4, 65536);
    hipLaunchKernelGGL(k_pw_copy, dim3((uint32_t)blocks), dim3(256), 0, s, a);
}

void launch_pair_check(const PairCheckArgs &a, hipStream_t s) {
    (void)hipMemsetAsync(a.status, 0xFF, 8, s);
    if (a.n_pairs == 0) return;
    const uint64_t blocks = std::min<uint64_t>((a.n_pairs + 3) / 4, 65536);
    hipLaunchKernelGGL(k_pm_check, dim3((uint32_t)blocks), dim3(256), 0, s, a);
}

void launch_pair_box(const unsigned long long *weave, const unsigned long long *check, uint64_t *box, hipStream_t s) {
    hipLaunchKernelGGL(k_pair_box, dim3(1), dim3(1), 0, s, weave, check, box);
}

void launch_pair_split(const PairSplitArgs &a, hipStream_t s) {
    if (a.n_pairs == 0) return;
    hipLaunchKernelGGL(k_ps_sizes, dim3((uint32_t)((a.n_pairs + 255) / 256)), dim3(256), 0, s, a.out_offs, a.n_pairs,
                       a.s1, a.s2);
    scan_excl_u64(a.s1, a.n_pairs, a.o1, a.tmp, s);
    scan_excl_u64(a.s2, a.n_pairs, a.o2, a.tmp, s);
    const uint64_t blocks = std::min<uint64_t>((2 * a.n_pairs + 3) / 4, 65536);
    hipLaunchKernelGGL(k_ps_copy, dim3((uint32_t)blocks), dim3(256), 0, s, a);
}

}  // namespace ntc
