// FASTQ quality scores, coder 1: a static order-1 rANS coder per block (qrans_core.h has the
// logic, DESIGN.md "Quality scores, rANS" the format).  Encode, over what k_q_gather and
// k_q_alpha (quality.hip) left in HBM -- the block's quality bytes, its presence words,
// alphabet and span count:
//   k_qr_hist    a workgroup takes kQRHistSpans spans: (context, symbol) counts in LDS, one
//                global atomic per non-zero count
//   k_qr_norm    one workgroup per block, one thread per row: the row normalised to 4096 and
//                kept as a cumulative row (the table of the body is its differences)
//   k_qr_encode  one lane per span, the block's cumulative rows in LDS: the qualities 8 bytes
//                per load, last to first; the bytes go backward from the end of the span's
//                scratch slot, a 32-bit word per store, so the stream stands forward
//   (scan of the span sizes)
//   k_qr_layout  per block the body's bytes and its 8-aligned place; the total to the mailbox
//   k_qr_place   one wave per span: its size and its stream to their place in the body; the
//                wave of a block's first span also writes the table and the padding
// Decode:
//   k_qr_flat    blocks of at most one symbol (no body): the count check and the fill
//   k_qr_decode  one lane per span, cumulative rows in LDS built from the body's table, the
//                symbol by binary search in the row, bytes gathered in a register and stored 8
//                at a time.  Every loop has a trip count fixed by the span's symbol count and
//                every byte read is clamped to the span: a damaged stream costs a wrong answer
//                and sets the status, nothing else.
// Workgroups and lanes take spans by their number over the whole call; the spans of one
// workgroup that lie in different blocks are taken block after block.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "qrans_core.h"

namespace ntc {

namespace {

constexpr uint32_t kQRHistSpans = 64;  // spans per workgroup of k_qr_hist
static_assert(kQRSlot % 8 == 0 && kQRSlot >= qr_span_bound(kQRSpan), "a slot holds the longest stream");
static_assert(kQRCumStride == 95 * kQRRow && kQRCountStride == 95 * kQRMaxSyms, "strides of qrans_core.h's rows");

__device__ __forceinline__ uint64_t umin(uint64_t x, uint64_t y) { return x < y ? x : y; }

__device__ __forceinline__ void q_fail(unsigned long long *status, uint64_t r) {
    atomicMin(status, (unsigned long long)(r << 8 | kErrFormat));
}

// 8 bytes from any address: two aligned loads (the arrays end in 64 bytes of slack)
__device__ __forceinline__ uint64_t load8(const uint8_t *p) {
    const uint64_t *q = (const uint64_t *)((uintptr_t)p & ~(uintptr_t)7);
    const uint32_t sh = 8 * (uint32_t)((uintptr_t)p & 7);
    const uint64_t lo = q[0];
    return sh ? lo >> sh | q[1] << (64 - sh) : lo;
}

// the block that holds span s: the last one whose first span is <= s (blocks without spans
// share their successor's first span; entry n holds the total)
template <class B>
__device__ __forceinline__ uint64_t block_of(const B *blocks, uint64_t n, uint64_t s) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (blocks[mid].span_off <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_qr_hist(QREncArgs a) {
    __shared__ uint32_t cnt[kQRCountStride];
    if (*a.q.status != ~0ull) return;  // a failed read: the call fails, no section is returned
    const QBlock *blocks = a.q.blocks;
    const uint64_t nb = a.q.n_blocks, total = blocks[nb].span_off;
    uint64_t s0 = (uint64_t)blockIdx.x * kQRHistSpans;
    const uint64_t send = umin(s0 + kQRHistSpans, total);
    while (s0 < send) {  // (the same for every thread)
        const uint64_t b = block_of(blocks, nb, s0);
        const QBlock *k = blocks + b;
        const uint64_t s1 = umin(send, blocks[b + 1].span_off);
        const uint32_t n = k->n_syms, cells = (n + 1) * n;
        const uint64_t p0 = k->p0, p1 = k->p1;
        for (uint32_t i = threadIdx.x; i < cells; i += 256) cnt[i] = 0;
        __syncthreads();
        const uint8_t *src = a.q.quals + k->q_off;
        const uint64_t nq = k->n_quals;
        for (uint64_t s = s0; s < s1; s++) {  // a span per pass: 8 qualities per thread
            const uint64_t i = (s - k->span_off) * kQRSpan + 8 * threadIdx.x;
            if (i >= nq) continue;
            const uint32_t live = (uint32_t)umin(8, nq - i);
            const uint64_t v = load8(src + i);
            uint32_t ctx = threadIdx.x ? q_rank(p0, p1, src[i - 1] & 0x7F) : n;
            for (uint32_t j = 0; j < 8; j++) {
                if (j >= live) break;
                const uint32_t sym = q_rank(p0, p1, (uint32_t)(v >> (8 * j)) & 0x7F);
                atomicAdd(&cnt[ctx * n + sym], 1u);
                ctx = sym;
            }
        }
        __syncthreads();
        uint32_t *out = a.counts + b * kQRCountStride;
        for (uint32_t i = threadIdx.x; i < cells; i += 256)
            if (cnt[i]) atomicAdd(&out[i], cnt[i]);
        __syncthreads();
        s0 = s1;
    }
}

// Row r of block b -> cumulative row r of a.cum (kQRRow entries, n_syms + 1 used)
__global__ __launch_bounds__(128) void k_qr_norm(QREncArgs a) {
    if (*a.q.status != ~0ull) return;
    const uint64_t b = blockIdx.x;
    const uint32_t n = a.q.blocks[b].n_syms, r = threadIdx.x;
    if (n <= 1 || r > n) return;
    uint16_t *row = a.cum + b * kQRCumStride + r * kQRRow;
    qr_normalise(a.counts + b * kQRCountStride + r * n, n, row + 1);
    row[0] = 0;
    uint32_t acc = 0;
    for (uint32_t s = 0; s < n; s++) {
        acc += row[s + 1];
        row[s + 1] = (uint16_t)acc;
    }
}

__global__ __launch_bounds__(64) void k_qr_encode(QREncArgs a) {
    __shared__ uint32_t tab32[kQRCumStride / 2];
    __shared__ uint8_t rk[128];
    if (*a.q.status != ~0ull) return;
    const uint16_t *tab = (const uint16_t *)tab32;
    const QBlock *blocks = a.q.blocks;
    const uint64_t nb = a.q.n_blocks, total = blocks[nb].span_off;
    const uint32_t lane = threadIdx.x;
    uint64_t s0 = (uint64_t)blockIdx.x * 64;
    const uint64_t send = umin(s0 + 64, total);
    while (s0 < send) {  // (the same for every lane)
        const uint64_t b = block_of(blocks, nb, s0);
        const QBlock *k = blocks + b;
        const uint64_t s1 = umin(send, blocks[b + 1].span_off);
        const uint32_t n = k->n_syms;
        const uint32_t *cum32 = (const uint32_t *)(a.cum + b * kQRCumStride);
        for (uint32_t i = lane; i < (n + 1) * (kQRRow / 2); i += 64) tab32[i] = cum32[i];
        rk[lane] = (uint8_t)q_rank(k->p0, k->p1, lane);
        rk[lane + 64] = (uint8_t)q_rank(k->p0, k->p1, lane + 64);
        __syncthreads();
        const uint64_t s = s0 + lane;
        if (s < s1) {
            const uint64_t base = (s - k->span_off) * kQRSpan;
            const uint32_t n_in = (uint32_t)umin(kQRSpan, k->n_quals - base);
            const uint8_t *src = a.q.quals + k->q_off + base;
            uint8_t *const end = a.scratch + (s + 1) * kQRSlot;  // 8-aligned
            uint8_t *p = end;
            uint32_t x = kQRL, acc = 0, na = 0;
            const auto emit = [&](uint32_t byte) {  // earlier bytes at higher addresses
                acc = acc << 8 | byte;
                if (++na == 4) {
                    p -= 4;
                    *(uint32_t *)p = acc;
                    na = 0;
                }
            };
            const uint32_t chunks = (n_in + 7) / 8;
            uint64_t cur = load8(src + 8 * (uint64_t)(chunks - 1));
            for (uint32_t c = chunks; c-- > 0;) {
                const uint64_t prev = c ? load8(src + 8 * (uint64_t)(c - 1)) : 0;
                const uint32_t live = n_in - 8 * c < 8 ? n_in - 8 * c : 8;
                for (uint32_t j = 8; j-- > 0;) {
                    if (j >= live) continue;
                    const uint32_t sym = rk[(uint32_t)(cur >> (8 * j)) & 0x7F];
                    const uint32_t ctx = j   ? rk[(uint32_t)(cur >> (8 * j - 8)) & 0x7F]
                                         : c ? rk[(uint32_t)(prev >> 56) & 0x7F]
                                             : n;
                    const uint16_t *row = tab + ctx * kQRRow;
                    const uint32_t cs = row[sym], f = row[sym + 1] - cs;
                    x = qr_encode_step(x, cs, f, emit);
                }
                cur = prev;
            }
            emit(x >> 24);
            emit((x >> 16) & 0xFF);
            emit((x >> 8) & 0xFF);
            emit(x & 0xFF);
            for (uint32_t t = na; t-- > 0;) *--p = (uint8_t)(acc >> (8 * t));
            a.sizes[s] = (uint64_t)(end - p);
        }
        __syncthreads();
        s0 = s1;
    }
}

// One workgroup: the call has few blocks (as k_q_alpha).
__global__ __launch_bounds__(256) void k_qr_layout(QREncArgs a) {
    if (*a.q.status != ~0ull) return;
    QBlock *blocks = a.q.blocks;
    const uint64_t nb = a.q.n_blocks;
    for (uint64_t b = threadIdx.x; b < nb; b += 256) {
        QBlock *k = blocks + b;
        const uint64_t f = k->span_off, l = blocks[b + 1].span_off;
        k->body_bytes = k->n_syms <= 1 ? 0 : qr_table_bytes(k->n_syms) + 4 * (l - f) + (a.offs[l] - a.offs[f]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t at = 0;
    for (uint64_t b = 0; b < nb; b++) {
        blocks[b].word_off = at / 8;
        at += (blocks[b].body_bytes + 7) & ~7ull;
    }
    blocks[nb].word_off = at / 8;
    a.q.box[kBoxQualWords] = at / 8;
}

__global__ __launch_bounds__(256) void k_qr_place(QREncArgs a) {
    if (*a.q.status != ~0ull) return;
    const QBlock *blocks = a.q.blocks;
    const uint64_t nb = a.q.n_blocks;
    const uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= blocks[nb].span_off) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = block_of(blocks, nb, s);
    const QBlock *k = blocks + b;
    const uint32_t n = k->n_syms;
    const uint64_t j = s - k->span_off, ns = blocks[b + 1].span_off - k->span_off, tb = qr_table_bytes(n);
    uint8_t *body = (uint8_t *)a.q.payload + k->word_off * 8;
    if (j == 0) {
        const uint16_t *cum = a.cum + b * kQRCumStride;
        uint16_t *t = (uint16_t *)body;
        for (uint32_t i = lane; i < (n + 1) * n; i += 64) {
            const uint32_t r = i / n, c = i % n;
            t[i] = (uint16_t)(cum[r * kQRRow + c + 1] - cum[r * kQRRow + c]);
        }
        const uint64_t pad = ((k->body_bytes + 7) & ~7ull) - k->body_bytes;
        if (lane < pad) body[k->body_bytes + lane] = 0;
    }
    const uint64_t size = a.sizes[s];
    if (lane == 0) ((uint32_t *)(body + tb))[j] = (uint32_t)size;
    uint8_t *dst = body + tb + 4 * ns + (a.offs[s] - a.offs[k->span_off]);
    const uint8_t *src = a.scratch + (s + 1) * kQRSlot - size;
    const uint64_t head = umin((0 - (uintptr_t)dst) & 7, size), words = (size - head) / 8;
    if (lane < head) dst[lane] = src[lane];
    for (uint64_t w = lane; w < words; w += 64) ((uint64_t *)(dst + head))[w] = load8(src + head + 8 * w);
    const uint64_t done = head + 8 * words;
    if (done + lane < size) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(256) void k_qr_flat(QRDecArgs a) {
    if (*a.status != ~0ull) return;  // the walk failed: the offsets are not to be trusted
    const QRDecBlock *k = a.blocks + blockIdx.x;
    if (k->n_syms > 1 || k->r0 > k->r1 || k->r1 > a.n_reads) return;
    const uint64_t at = a.offs[k->r0] - a.offs[0], have = a.offs[k->r1] - a.offs[k->r0];
    if (have != k->n_quals) {
        if (threadIdx.x == 0) q_fail(a.status, k->r0);
        return;
    }
    for (uint64_t i = threadIdx.x; i < k->n_quals; i += 256) a.quals[at + i] = k->alphabet[0];
}

__global__ __launch_bounds__(64) void k_qr_decode(QRDecArgs a) {
    __shared__ uint16_t tab[kQRCumStride];
    __shared__ uint8_t alpha[96];
    if (*a.status != ~0ull) return;
    const QRDecBlock *blocks = a.blocks;
    const uint64_t nb = a.n_blocks, total = a.n_spans;
    const uint32_t lane = threadIdx.x;
    uint64_t s0 = (uint64_t)blockIdx.x * 64;
    const uint64_t send = umin(s0 + 64, total);
    while (s0 < send) {  // (the same for every lane)
        const uint64_t b = block_of(blocks, nb, s0);
        const QRDecBlock *k = blocks + b;
        const uint64_t s1 = umin(send, blocks[b + 1].span_off);
        const uint32_t n = k->n_syms;  // 2 .. 94: the host checked, and a block of fewer has no span
        const uint16_t *ft = (const uint16_t *)(a.payload + k->body_off);
        for (uint32_t r = lane; r <= n; r += 64) {
            uint16_t *row = tab + r * kQRRow;
            uint32_t acc = 0;
            row[0] = 0;
            for (uint32_t c = 0; c < n; c++) {
                acc += ft[r * n + c];
                row[c + 1] = (uint16_t)acc;
            }
        }
        alpha[lane] = k->alphabet[lane];
        if (lane < 32) alpha[lane + 64] = k->alphabet[lane + 64];
        __syncthreads();
        const uint64_t s = s0 + lane, j = s - k->span_off;
        const bool sound = k->r0 <= k->r1 && k->r1 <= a.n_reads;  // (the host checked)
        if (s < s1 && sound) {
            const uint64_t have = a.offs[k->r1] - a.offs[k->r0];
            if (have != k->n_quals) {
                if (j == 0) q_fail(a.status, k->r0);
            } else {
                const uint64_t base = j * kQRSpan;
                const uint32_t n_in = (uint32_t)umin(kQRSpan, k->n_quals - base);
                uint64_t pos = a.span_at[2 * s];
                const uint64_t en = a.span_at[2 * s + 1];
                bool bad = false;
                const auto next = [&]() -> uint32_t {  // clamped to the span
                    if (pos < en) return a.payload[pos++];
                    bad = true;
                    return 0;
                };
                uint32_t x = next();
                x |= next() << 8;
                x |= next() << 16;
                x |= next() << 24;
                if (x < kQRL || x >> 31) bad = true;
                const uint64_t d0 = a.offs[k->r0] - a.offs[0] + base;  // the span's first byte in quals
                uint64_t acc = 0;
                uint32_t ctx = n, first = (uint32_t)(d0 & 7);
                for (uint32_t i = 0; i < n_in; i++) {
                    const uint16_t *row = tab + ctx * kQRRow;
                    const uint32_t slot = x & (kQRTotal - 1);
                    if (slot >= row[n]) bad = true;  // a zero row
                    const uint32_t sym = qr_find(row, n, slot);
                    const uint32_t cs = row[sym], f = row[sym + 1] - cs;
                    x = qr_decode_step(x, cs, f);
                    if (!qr_refill(x, next)) bad = true;
                    ctx = sym;
                    const uint64_t d = d0 + i;
                    const uint32_t o = (uint32_t)(d & 7);
                    acc |= (uint64_t)alpha[sym] << (8 * o);
                    if (o == 7 || i + 1 == n_in) {
                        if (first == 0 && o == 7) {
                            *(uint64_t *)(a.quals + (d & ~7ull)) = acc;
                        } else {
                            for (uint32_t t = first; t <= o; t++) a.quals[(d & ~7ull) + t] = (uint8_t)(acc >> (8 * t));
                        }
                        acc = 0;
                        first = 0;
                    }
                }
                if (x != kQRL || pos != en) bad = true;
                if (bad) q_fail(a.status, k->r0);
            }
        }
        __syncthreads();
        s0 = s1;
    }
}

}  // namespace

uint64_t qr_spans_max(uint64_t total, uint64_t n_blocks) { return total / kQRSpan + n_blocks; }

// every body rounded up to 8: table, span sizes, and streams of at most qr_span_bound bytes
uint64_t qr_payload_bytes_max(uint64_t total, uint64_t n_blocks) {
    return total + total / 2 + 8 * qr_spans_max(total, n_blocks) + n_blocks * (qr_table_bytes(kQRMaxSyms) + 8);
}

void launch_quality_rans(const QREncArgs &a, hipStream_t s) {
    if (a.q.n_blocks == 0) return;
    const uint64_t S = a.spans_max;
    (void)hipMemsetAsync(a.counts, 0, a.q.n_blocks * kQRCountStride * 4, s);  // a failure shows in the caller's hipGetLastError
    (void)hipMemsetAsync(a.sizes, 0, (S + 1) * 8, s);
    hipLaunchKernelGGL(k_qr_hist, dim3((uint32_t)((S + kQRHistSpans - 1) / kQRHistSpans)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_qr_norm, dim3((uint32_t)a.q.n_blocks), dim3(128), 0, s, a);
    hipLaunchKernelGGL(k_qr_encode, dim3((uint32_t)((S + 63) / 64)), dim3(64), 0, s, a);
    scan_excl_u64(a.sizes, S, a.offs, a.tmp, s);
    hipLaunchKernelGGL(k_qr_layout, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_qr_place, dim3((uint32_t)((S + 3) / 4)), dim3(256), 0, s, a);
}

void launch_quality_rans_decode(const QRDecArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    hipLaunchKernelGGL(k_qr_flat, dim3((uint32_t)a.n_blocks), dim3(256), 0, s, a);
    if (a.n_spans) hipLaunchKernelGGL(k_qr_decode, dim3((uint32_t)((a.n_spans + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace ntc
