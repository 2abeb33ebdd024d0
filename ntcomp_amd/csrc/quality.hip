// FASTQ quality scores on the GPU (quality_core.h has the logic, DESIGN.md "Quality scores").
// Encode, over the text fastq.hip has parsed (newline table + read offsets):
//   k_q_gather  one wave per record: the quality line through the mode's 256-entry table to
//               a contiguous array at the read's base offset; the two checks (as many
//               qualities as bases kept, every byte in '!'..'~'); the block's presence map
//               (LDS first, then one atomicOr per word and workgroup)
//   k_q_alpha   per block: alphabet, width, counts, payload word offset; totals and the
//               status to the host mailbox (no sync of its own)
//   k_q_smooth  option "quality_smooth" only, between k_q_gather and k_q_alpha once the encode
//               has its records: one wave per read at a time, the rule of qsmooth_core.h in place, the
//               presence maps rebuilt from the smoothed bytes, the bytes replaced counted
//   k_q_pack    one wave per span of kQSpan qualities: 8 bytes per lane and load (512
//               contiguous bytes per wave), ranks from the presence words, the lanes of
//               one output word combined by shuffles, contiguous 64-bit stores
// Decode:
//   k_q_unpack  codes -> bytes at the decoded reads' offsets
//   k_fastq_sizes, (scan), k_fastq   "@seq.N\n" bases "\n+\n" qualities "\n", one wave per
//               read, as fasta.hip formats FASTA
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "qrans_core.h"
#include "qsmooth_core.h"
#include "quality_core.h"
#include "window_core.h"

namespace ntc {

namespace {

constexpr uint32_t kQChunk = 64;   // records per workgroup of k_q_gather (16 per wave)
constexpr uint32_t kQSpan = 2048;  // qualities per wave of k_q_pack (4 loads of 8 B per lane)
constexpr uint32_t kQTile = 1024;  // qualities per workgroup of k_q_unpack
static_assert(kQSpan == kQRSpan, "k_q_alpha counts the spans of both coders");

__device__ __forceinline__ uint64_t umin(uint64_t x, uint64_t y) { return x < y ? x : y; }

__device__ __forceinline__ void q_fail(unsigned long long *status, uint64_t r) {
    atomicMin(status, (unsigned long long)(r << 8 | kErrFormat));
}

// The chunk's records lie in one block, so the workgroup ORs into one presence map.
__global__ __launch_bounds__(256) void k_q_gather(QEncArgs a) {
    __shared__ uint8_t tab[256];
    __shared__ uint32_t pres[4];
    tab[threadIdx.x] = (uint8_t)q_table(a.mode, threadIdx.x);
    if (threadIdx.x < 4) pres[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t cpb = (a.block_reads + kQChunk - 1) / kQChunk;
    const uint64_t b = blockIdx.x / cpb, c = blockIdx.x % cpb;
    const uint64_t r0 = b * a.block_reads + c * kQChunk;
    const uint64_t r1 = umin(umin(r0 + kQChunk, (b + 1) * a.block_reads), a.n_reads);
    const uint64_t n_nl = *a.n_nl_p;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = r0 + (threadIdx.x >> 6); r < r1; r += 4) {
        const uint64_t q0 = (uint64_t)a.nl[4 * r + 2] + 1;
        const uint64_t q1 = 4 * r + 3 < n_nl ? (uint64_t)a.nl[4 * r + 3] : a.n_raw;
        const uint64_t len = q1 - q0 - (q1 > q0 && a.raw[q1 - 1] == '\r');
        const uint64_t o = a.offs[r];
        bool bad = len != a.offs[r + 1] - o;  // then nothing is written: the array has room for the bases only
        if (!bad) {
            for (uint64_t i = lane; i < len; i += 64) {
                const uint32_t t = tab[a.raw[q0 + i]];
                if (!t) {
                    bad = true;
                    continue;
                }
                a.quals[o + i] = (uint8_t)t;
                if (!((((volatile uint32_t *)pres)[t >> 5] >> (t & 31)) & 1)) atomicOr(&pres[t >> 5], 1u << (t & 31));
            }
        }
        if (__any(bad) && lane == 0) q_fail(a.status, r);
    }
    __syncthreads();
    if (threadIdx.x < 4 && pres[threadIdx.x]) atomicOr(&a.pres[4 * b + threadIdx.x], pres[threadIdx.x]);
}

// One workgroup: the call has few blocks.  blocks[n_blocks] carries the totals.
__global__ __launch_bounds__(256) void k_q_alpha(QEncArgs a) {
    for (uint64_t b = threadIdx.x; b < a.n_blocks; b += 256) {
        const uint64_t r0 = b * a.block_reads, r1 = umin(r0 + a.block_reads, a.n_reads);
        QBlock k{};
        k.p0 = (uint64_t)a.pres[4 * b] | (uint64_t)a.pres[4 * b + 1] << 32;
        k.p1 = (uint64_t)a.pres[4 * b + 2] | (uint64_t)a.pres[4 * b + 3] << 32;
        k.n_quals = a.offs[r1] - a.offs[r0];
        k.q_off = a.offs[r0];
        k.n_syms = q_alphabet(k.p0, k.p1, k.alphabet);
        k.w = q_width(k.n_syms);
        k.n_words = q_words(k.n_quals, k.w);
        a.blocks[b] = k;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t words = 0, spans = 0;
    for (uint64_t b = 0; b < a.n_blocks; b++) {
        QBlock *k = a.blocks + b;
        k->word_off = words;
        k->span_off = spans;
        words += k->n_words;
        spans += k->w ? (k->n_quals + kQSpan - 1) / kQSpan : 0;
    }
    a.blocks[a.n_blocks].word_off = words;
    a.blocks[a.n_blocks].span_off = spans;
    a.box[kBoxQualStatus] = *a.status;
    a.box[kBoxQualWords] = words;
}

// 8 bytes from any address: two aligned loads (the arrays end in 64 bytes of slack)
__device__ __forceinline__ uint64_t load8(const uint8_t *p) {
    const uint64_t *q = (const uint64_t *)((uintptr_t)p & ~(uintptr_t)7);
    const uint32_t sh = 8 * (uint32_t)((uintptr_t)p & 7);
    const uint64_t lo = q[0];
    return sh ? lo >> sh | q[1] << (64 - sh) : lo;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    return (uint64_t)__shfl_xor((uint32_t)v, o) | (uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32;
}

__global__ __launch_bounds__(256) void k_q_pack(QEncArgs a) {
    if (*a.status != ~0ull) return;  // a failed read: the call fails, no section is returned
    const uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.blocks[a.n_blocks].span_off) return;
    uint64_t lo = 0, hi = a.n_blocks;  // the last block whose first span is <= s (blocks of width 0 have none)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (a.blocks[mid].span_off <= s) lo = mid;
        else hi = mid;
    }
    const QBlock *k = a.blocks + lo;
    const uint64_t nq = k->n_quals, n_words = k->n_words, p0 = k->p0, p1 = k->p1;
    const uint32_t w = k->w, lane = threadIdx.x & 63;
    if (!w) return;  // (a block of width 0 has no spans)
    const uint32_t per = 8 / w;  // lanes that share an output word
    const uint8_t *src = a.quals + k->q_off;
    uint64_t *dst = a.payload + k->word_off;
    const uint64_t base = (s - k->span_off) * kQSpan;
    for (uint32_t it = 0; it < kQSpan / 512; it++) {
        if (base + it * 512 >= nq) break;  // (the same for every lane: all take part in the shuffles)
        const uint64_t i = base + it * 512 + 8 * lane;
        const uint32_t live = i < nq ? (uint32_t)umin(8, nq - i) : 0;
        uint64_t bits = live ? q_pack8(load8(src + i), live, p0, p1, w) << ((lane % per) * 8 * w) : 0;
        for (uint32_t o = 1; o < per; o <<= 1) bits |= shfl_xor64(bits, (int)o);
        const uint64_t word = i * w >> 6;
        if (lane % per == 0 && word < n_words) dst[word] = bits;
    }
}

// Smoothing (qsmooth_core.h): a workgroup takes kQsReads consecutive reads of one block, a wave
// one read at a time.  The read's records come kQsChunk at a time, a record per lane; a wave
// scan of their lengths gives the chunk's entries, which the wave keeps in its own row of
// LDS.  The lanes then sweep the chunk's qualities an aligned 8-byte word each: the word's
// trusted mask from the entries, the rule, the presence bits of what is left.  A word that
// lies wholly inside the chunk is stored whole; a word at either edge is shared with the
// neighbouring read or chunk, whose wave owns the other bytes, and has its replaced bytes
// stored one by one.  No byte is written by two waves, and none is read after another wave
// may have written it, so the pass needs no ordering between waves.  Presence bits and the
// count gather in registers, then in LDS, and reach memory once per workgroup: a million
// atomics on one word take 21 ms.
constexpr uint32_t kQsReads = 128;

__global__ __launch_bounds__(256) void k_q_smooth(QSmoothArgs a) {
    __shared__ uint32_t ents[4][kQsChunk];
    __shared__ uint32_t pres[4];
    __shared__ unsigned long long total;
    if (*a.q.status != ~0ull) return;  // a failed read: the call fails, no section is returned
    if (threadIdx.x < 4) pres[threadIdx.x] = 0;
    if (threadIdx.x == 4) total = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    uint32_t *ent = ents[threadIdx.x >> 6];
    const uint32_t floor = qs_floor(a.q.mode), target = qs_target(a.q.mode, a.to);
    const uint32_t cpb = (a.q.block_reads + kQsReads - 1) / kQsReads;
    const uint64_t b = blockIdx.x / cpb, c0 = blockIdx.x % cpb;
    const uint64_t r0 = b * a.q.block_reads + c0 * kQsReads;
    const uint64_t r1 = umin(umin(r0 + kQsReads, (b + 1) * a.q.block_reads), a.q.n_reads);
    uint64_t p0 = 0, p1 = 0;
    uint32_t replaced = 0;
    for (uint64_t r = r0 + (threadIdx.x >> 6); r < r1; r += 4) {
        const uint64_t o = a.q.offs[r], j0 = a.roffs[r], m = a.roffs[r + 1] - j0;
        uint64_t hi = a.q.offs[r + 1] - o;  // the chunk's records end here
        for (uint64_t c = 0; c < m; c += kQsChunk) {
            const uint32_t cnt = (uint32_t)umin(kQsChunk, m - c);
            const uint64_t rec = lane < cnt ? a.recs[j0 + c + lane] : 0;
            uint32_t inc = lane < cnt ? qs_rec_len(rec) : 0;
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(inc, d, 64);
                if (lane >= d) inc += t;
            }
            const uint32_t span = __shfl(inc, 63, 64);
            if (span > hi) break;  // (records that outrun the read: the encode did not write them)
            if (span == 0) continue;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the last chunk's reads of ent are done
            __builtin_amdgcn_wave_barrier();
            if (lane < cnt) ent[lane] = qs_entry(span, inc, rec, a.m);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint64_t lo = o + (hi - span), end = o + hi;  // the chunk's bytes of quals
            for (uint64_t at = (lo & ~7ull) + 8 * lane; at < end; at += 512) {
                uint64_t live, changed;
                const uint64_t mask = qs_word_mask(ent, cnt, span, (int64_t)at - (int64_t)lo, &live);
                uint64_t *word = (uint64_t *)(a.q.quals + at);
                const uint64_t v = qs_apply(*word, mask, floor, target, &changed);
                qs_presence(v, live, &p0, &p1);
                if (!changed) continue;
                replaced += q_popc(changed) >> 3;
                if (live == ~0ull) {
                    *word = v;
                } else {
                    for (uint32_t j = 0; j < 8; j++)
                        if ((changed >> (8 * j)) & 1) a.q.quals[at + j] = (uint8_t)target;
                }
            }
            hi -= span;
        }
    }
    for (int d = 1; d < 64; d <<= 1) {
        p0 |= shfl_xor64(p0, d);
        p1 |= shfl_xor64(p1, d);
        replaced += __shfl_xor(replaced, d);
    }
    if (lane == 0) {
        const uint32_t w[4] = {(uint32_t)p0, (uint32_t)(p0 >> 32), (uint32_t)p1, (uint32_t)(p1 >> 32)};
        for (uint32_t i = 0; i < 4; i++)
            if (w[i]) atomicOr(&pres[i], w[i]);
        if (replaced) atomicAdd(&total, (unsigned long long)replaced);
    }
    __syncthreads();
    // (a stale read of the block's map only costs an atomic that adds nothing)
    if (threadIdx.x < 4 && (pres[threadIdx.x] & ~a.q.pres[4 * b + threadIdx.x])) atomicOr(&a.q.pres[4 * b + threadIdx.x], pres[threadIdx.x]);
    if (threadIdx.x == 4 && total) atomicAdd(a.count, total);
}

// Workgroup t of block b: qualities [t kQTile, ...) of the block, a byte per thread and store
// (64 contiguous bytes per wave).  Nothing is written for a block whose count differs from
// the bases the walk produced for its reads.
__global__ __launch_bounds__(256) void k_q_unpack(QDecArgs a) {
    if (*a.status != ~0ull) return;  // the walk failed: the offsets are not to be trusted
    const uint64_t b = blockIdx.x / a.tiles, t = blockIdx.x % a.tiles;
    const QDecBlock *k = a.blocks + b;
    if (k->r0 > k->r1 || k->r1 > a.n_reads) return;  // (the host checked)
    const uint64_t at = a.offs[k->r0] - a.offs[0], have = a.offs[k->r1] - a.offs[k->r0];
    if (have != k->n_quals) {
        if (t == 0 && threadIdx.x == 0) q_fail(a.status, k->r0);
        return;
    }
    const uint64_t *src = a.payload + k->word_off;
    for (uint32_t j = 0; j < kQTile / 256; j++) {
        const uint64_t i = t * kQTile + j * 256 + threadIdx.x;
        if (i >= k->n_quals) return;
        const uint32_t code = k->w ? q_code_at(src, i, k->w) : 0;
        if (code >= k->n_syms) q_fail(a.status, k->r0);
        else a.quals[at + i] = k->alphabet[code];
    }
}

__device__ __forceinline__ uint32_t ndigits(uint64_t x) {
    uint32_t d = 1;
    while (x >= 10) {
        x /= 10;
        d++;
    }
    return d;
}

// as k_fasta_sizes: every size is 0 unless the status is clear (walk, patch and unpack)
__global__ __launch_bounds__(256) void k_fastq_sizes(const uint64_t *offs, uint64_t n, uint64_t first_id,
                                                     const unsigned long long *status, uint64_t *sizes) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    sizes[r] = *status != ~0ull ? 0 : 5 + ndigits(first_id + r) + 1 + 2 * (offs[r + 1] - offs[r]) + 4;
}

// W: the call has a window (window.hip zeroed the sizes outside it): reads without a record are
// skipped.  W = false is the kernel as it was.
template <bool W>
__global__ __launch_bounds__(256) void k_fastq(const uint8_t *bases, const uint8_t *quals, const uint64_t *offs,
                                               uint64_t n, uint64_t first_id, const uint64_t *out_offs,
                                               uint64_t out_cap, uint8_t *out) {
    if (out_offs[n] == 0 || out_offs[n] > out_cap) return;  // a failed call (sizes 0) or a short buffer
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
    const uint64_t o0 = offs[0];
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); r < n; r += waves) {
        if (W && w_skips(out_offs[r], out_offs[r + 1])) continue;
        const uint64_t b = offs[r] - o0, len = offs[r + 1] - offs[r];
        uint64_t o = out_offs[r];
        const uint64_t id = first_id + r;
        const uint32_t nd = ndigits(id);
        if (lane < 5 + nd + 1) {
            uint8_t ch;
            if (lane < 5) {
                ch = (uint8_t)"@seq."[lane];
            } else if (lane < 5 + nd) {
                uint64_t x = id;
                for (uint32_t t = lane - 5 + 1; t < nd; t++) x /= 10;  // digit lane - 5 from the left
                ch = (uint8_t)('0' + x % 10);
            } else {
                ch = '\n';
            }
            out[o + lane] = ch;
        }
        o += 5 + nd + 1;
        for (uint64_t i = lane; i < len; i += 64) out[o + i] = bases[b + i];
        if (lane < 3) out[o + len + lane] = (uint8_t)"\n+\n"[lane];
        o += len + 3;
        for (uint64_t i = lane; i < len; i += 64) out[o + i] = quals[b + i];
        if (lane == 0) out[o + len] = '\n';
    }
}

}  // namespace

uint64_t q_payload_words_max(uint64_t total, uint64_t n_blocks) { return total / 8 + n_blocks + 1; }

void launch_quality_gather(const QEncArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    (void)hipMemsetAsync(a.pres, 0, a.n_blocks * 16, s);  // a failure shows in the caller's hipGetLastError
    (void)hipMemsetAsync(a.status, 0xFF, 8, s);
    const uint64_t cpb = (a.block_reads + kQChunk - 1) / kQChunk;
    hipLaunchKernelGGL(k_q_gather, dim3((uint32_t)(a.n_blocks * cpb)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_q_alpha, dim3(1), dim3(256), 0, s, a);
}

void launch_quality_pack(const QEncArgs &a, uint64_t total, hipStream_t s) {
    if (a.n_blocks == 0) return;
    launch_quality_gather(a, s);
    const uint64_t spans = total / kQSpan + a.n_blocks;  // at most: a block's last span may be short
    hipLaunchKernelGGL(k_q_pack, dim3((uint32_t)((spans + 3) / 4)), dim3(256), 0, s, a);
}

void launch_quality_lines(const QEncArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    (void)hipMemsetAsync(a.pres, 0, a.n_blocks * 16, s);  // a failure shows in the caller's hipGetLastError
    (void)hipMemsetAsync(a.status, 0xFF, 8, s);
    const uint64_t cpb = (a.block_reads + kQChunk - 1) / kQChunk;
    hipLaunchKernelGGL(k_q_gather, dim3((uint32_t)(a.n_blocks * cpb)), dim3(256), 0, s, a);
}

void launch_quality_smooth(const QSmoothArgs &a, hipStream_t s) {
    if (a.q.n_blocks == 0) return;
    (void)hipMemsetAsync(a.q.pres, 0, a.q.n_blocks * 16, s);
    (void)hipMemsetAsync(a.count, 0, 8, s);
    const uint64_t cpb = (a.q.block_reads + kQsReads - 1) / kQsReads;
    hipLaunchKernelGGL(k_q_smooth, dim3((uint32_t)(a.q.n_blocks * cpb)), dim3(256), 0, s, a);
}

void launch_quality_alpha(const QEncArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    hipLaunchKernelGGL(k_q_alpha, dim3(1), dim3(256), 0, s, a);
}

void launch_quality_spans(const QEncArgs &a, uint64_t total, hipStream_t s) {
    if (a.n_blocks == 0) return;
    const uint64_t spans = total / kQSpan + a.n_blocks;  // at most: a block's last span may be short
    hipLaunchKernelGGL(k_q_pack, dim3((uint32_t)((spans + 3) / 4)), dim3(256), 0, s, a);
}

void launch_quality_unpack(const QDecArgs &a, hipStream_t s) {
    if (a.n_blocks == 0 || a.tiles == 0) return;
    hipLaunchKernelGGL(k_q_unpack, dim3((uint32_t)(a.n_blocks * a.tiles)), dim3(256), 0, s, a);
}

// at least one workgroup per block: an empty block's count is checked too
uint64_t quality_unpack_tiles(uint64_t max_quals) { return max_quals ? (max_quals + kQTile - 1) / kQTile : 1; }

void launch_fastq_text(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offs, uint64_t n,
                       uint64_t first_id, const unsigned long long *d_status, uint64_t *sizes, uint64_t *out_offs,
                       uint64_t *tmp, uint8_t *out, uint64_t out_cap, hipStream_t s, uint64_t w_first, uint64_t w_count) {
    if (!n) return;
    hipLaunchKernelGGL(k_fastq_sizes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_offs, n, first_id,
                       d_status, sizes);
    if (w_count) launch_window_sizes(sizes, n, w_first, w_count, s);
    scan_excl_u64(sizes, n, out_offs, tmp, s);
    const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, 65536);
    hipLaunchKernelGGL(w_count ? k_fastq<true> : k_fastq<false>, dim3((uint32_t)blocks), dim3(256), 0, s, d_bases, d_quals,
                       d_offs, n, first_id, out_offs, out_cap, out);
}

}  // namespace ntc
