// FASTQ read names on the GPU (names_core.h has the logic, DESIGN.md "Read names").
// Encode, over the text fastq.hip has parsed (raw bytes + newline table):
//   k_n_measure  one wave per record: the name's span (mode id: the cut by ballot + ctz), pre
//                and suf against the record before it in 64-byte ballot steps, forwards and
//                backwards; len, pre, suf and the mid count; a name past NTC_NAME_MAX fails
//   (scan x 2)   exclusive scans of len and of the mid counts
//   k_n_blocks   one workgroup: the per-block table, payload offsets; the totals and the
//                status to the host mailbox (no sync of its own)
//   k_n_emit     one wave per group of 64 reads: the three columns (a lane per read) and the
//                mids (lanes across bytes) into the section's place, zero padding at its end
// Decode:
//   k_n_lens     a thread per read: its columns against the per-read conditions -> len, mid
//   (scan x 2)   -> where each name and each mid starts
//   k_n_sums     a thread per section: mids and names sum to the meta
//   k_n_expand   one wave per group, sequential over its reads, lanes across bytes; the
//                previous name stays in LDS (two buffers per wave)
//   k_named_sizes, (scan), k_named   ">name\n" bases "\n", or "@name\n" bases "\n+\n"
//                qualities "\n"; one wave per read, as fasta.hip formats FASTA
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "names_core.h"
#include "window_core.h"

namespace ntc {

namespace {

__device__ __forceinline__ uint64_t umin(uint64_t x, uint64_t y) { return x < y ? x : y; }

__device__ __forceinline__ void n_fail(unsigned long long *status, uint64_t r) {
    atomicMin(status, (unsigned long long)(r << 8 | kErrFormat));
}

struct NSpan {
    uint64_t s, len;  // first byte in raw, bytes (mode id: after the cut)
};
// the name of record r (wave-uniform; every lane takes part in the ballots)
__device__ __forceinline__ NSpan n_span(const NEncArgs &a, uint64_t r, uint32_t lane) {
    const uint64_t h0 = r ? (uint64_t)a.nl[4 * r - 1] + 1 : 0, e = a.nl[4 * r];
    NSpan f;
    f.s = umin(h0 + 1, e);  // (the parse saw '@' at h0)
    f.len = e - f.s;
    if (f.len && a.raw[e - 1] == '\r') f.len--;
    if (a.mode == kNId) {
        for (uint64_t b = 0; b < f.len; b += 64) {
            const uint64_t i = b + lane;
            const uint64_t m = __ballot(i < f.len && n_is_cut(a.raw[f.s + i]));
            if (m) {
                f.len = b + n_ctz(m);
                break;
            }
        }
    }
    return f;
}

__global__ __launch_bounds__(256) void k_n_measure(NEncArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n_reads; r += waves) {
        const NSpan f = n_span(a, r, lane);
        if (f.len > kNMax) {
            if (lane == 0) {
                n_fail(a.status, r);
                a.start[r] = (uint32_t)f.s;
                a.len[r] = a.mid[r] = 0;
                a.ps[r] = a.ps[a.n_reads + r] = 0;
            }
            continue;
        }
        const uint32_t len = (uint32_t)f.len;
        uint32_t pre = 0, suf = 0;
        if ((r % a.block_reads) % kNGroup != 0) {
            const NSpan p = n_span(a, r - 1, lane);
            const uint32_t plen = (uint32_t)umin(p.len, kNMax);  // (longer: the call fails there)
            const uint32_t lim = n_pre_limit(plen, len);
            for (uint32_t b = 0; b < lim; b += 64) {
                const uint32_t live = lim - b < 64 ? lim - b : 64;
                const uint64_t eq = __ballot(lane < live && a.raw[p.s + b + lane] == a.raw[f.s + b + lane]);
                const uint32_t k = n_run(eq, live);
                pre += k;
                if (k < live) break;
            }
            const uint32_t slim = n_suf_limit(plen, len, pre);
            for (uint32_t b = 0; b < slim; b += 64) {
                const uint32_t live = slim - b < 64 ? slim - b : 64;
                const uint64_t eq = __ballot(lane < live && a.raw[p.s + plen - 1 - b - lane] == a.raw[f.s + len - 1 - b - lane]);
                const uint32_t k = n_run(eq, live);
                suf += k;
                if (k < live) break;
            }
        }
        if (lane == 0) {
            a.start[r] = (uint32_t)f.s;
            a.len[r] = len;
            a.mid[r] = len - pre - suf;
            a.ps[r] = (uint8_t)pre;
            a.ps[a.n_reads + r] = (uint8_t)suf;
        }
    }
}

// One workgroup: the call has few blocks.  blocks[n_blocks] carries the total.
__global__ __launch_bounds__(256) void k_n_blocks(NEncArgs a) {
    for (uint64_t b = threadIdx.x; b < a.n_blocks; b += 256) {
        const uint64_t r0 = b * a.block_reads, r1 = umin(r0 + a.block_reads, a.n_reads);
        NBlock k{};
        k.n_reads = r1 - r0;
        k.name_bytes = a.len_off[r1] - a.len_off[r0];
        k.mid_bytes = a.mid_off[r1] - a.mid_off[r0];
        k.payload_bytes = n_payload_bytes(k.n_reads, k.mid_bytes);
        a.blocks[b] = k;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t bytes = 0;
    for (uint64_t b = 0; b < a.n_blocks; b++) {
        a.blocks[b].payload_off = bytes;
        bytes += a.blocks[b].payload_bytes;
    }
    a.blocks[a.n_blocks].payload_off = bytes;
    a.box[kBoxNameStatus] = *a.status;
    a.box[kBoxNameBytes] = bytes;
}

__global__ __launch_bounds__(256) void k_n_emit(NEncArgs a) {
    if (*a.status != ~0ull) return;  // a name too long: the call fails, no section is returned
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t gpb = (a.block_reads + kNGroup - 1) / kNGroup;
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t b = g / gpb, i0 = (g % gpb) * kNGroup;
    if (b >= a.n_blocks) return;
    const NBlock k = a.blocks[b];
    if (i0 >= k.n_reads) return;
    const uint64_t r0 = b * a.block_reads, n = k.n_reads;
    uint8_t *sec = a.payload + k.payload_off;  // 8-byte aligned
    const uint32_t cnt = (uint32_t)umin(kNGroup, n - i0);
    uint32_t m_l = 0, s_l = 0;
    uint64_t o_l = 0;
    if (lane < cnt) {
        const uint64_t r = r0 + i0 + lane;
        const uint32_t pre = a.ps[r];
        ((uint16_t *)sec)[i0 + lane] = (uint16_t)a.len[r];
        sec[2 * n + i0 + lane] = (uint8_t)pre;
        sec[3 * n + i0 + lane] = a.ps[a.n_reads + r];
        m_l = a.mid[r];
        s_l = a.start[r] + pre;
        o_l = a.mid_off[r] - a.mid_off[r0];
    }
    uint8_t *mids = sec + 4 * n;
    for (uint32_t t = 0; t < cnt; t++) {
        const uint32_t m = __shfl(m_l, (int)t), s = __shfl(s_l, (int)t);
        const uint64_t o = (uint64_t)__shfl((uint32_t)o_l, (int)t) | (uint64_t)__shfl((uint32_t)(o_l >> 32), (int)t) << 32;
        for (uint32_t j = lane; j < m; j += 64) mids[o + j] = a.raw[(uint64_t)s + j];
    }
    if (i0 + kNGroup >= n) {  // the block's last group pads the section
        const uint64_t end = 4 * n + k.mid_bytes;
        if (end + lane < k.payload_bytes) sec[end + lane] = 0;
    }
}

// ---- decode ---------------------------------------------------------------------------

// the section that holds read r (the host checked that the sections cover [0, n_reads) in order)
__device__ __forceinline__ uint64_t n_block_of(const NDecArgs &a, uint64_t r) {
    uint64_t lo = 0, hi = a.n_blocks;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (a.blocks[mid].r0 <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the columns of section k lie inside the payload (the host checked; checked again here)
__device__ __forceinline__ bool n_sec_ok(const NDecArgs &a, const NDecBlock &k) {
    if (k.r1 < k.r0 || k.r1 > a.n_reads || (k.payload_off & 7) || k.payload_off > a.payload_bytes) return false;
    const uint64_t room = a.payload_bytes - k.payload_off, n = k.r1 - k.r0;
    return n <= room / 4 && k.mid_bytes <= room - 4 * n;
}

__global__ __launch_bounds__(256) void k_n_lens(NDecArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_reads) return;
    uint32_t len = 0, mid = 0;
    const NDecBlock k = a.blocks[n_block_of(a, r)];
    if (!n_sec_ok(a, k) || r < k.r0 || r >= k.r1) {
        n_fail(a.status, r);
    } else {
        const uint8_t *sec = a.payload + k.payload_off;
        const uint64_t n = k.r1 - k.r0, i = r - k.r0;
        const uint32_t l = ((const uint16_t *)sec)[i], pre = sec[2 * n + i], suf = sec[3 * n + i];
        const uint32_t plen = i % kNGroup ? ((const uint16_t *)sec)[i - 1] : 0;
        if (!n_read_ok((uint32_t)(i % kNGroup), l, pre, suf, plen)) {
            n_fail(a.status, r);
        } else {
            len = l;
            mid = l - pre - suf;
        }
    }
    a.len[r] = len;
    a.mid[r] = mid;
}

__global__ __launch_bounds__(256) void k_n_sums(NDecArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.n_blocks) return;
    const NDecBlock k = a.blocks[b];
    if (!n_sec_ok(a, k)) {
        n_fail(a.status, k.r0);
        return;
    }
    if (a.mid_off[k.r1] - a.mid_off[k.r0] != k.mid_bytes || a.name_off[k.r1] - a.name_off[k.r0] != k.name_bytes)
        n_fail(a.status, k.r0);
}

__global__ __launch_bounds__(256) void k_n_expand(NDecArgs a, uint64_t gmax) {
    __shared__ uint8_t buf[4][2][kNMax + 1];
    if (*a.status != ~0ull) return;  // the walk or a section failed: nothing is expanded
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t g = (uint64_t)blockIdx.x * 4 + wave;
    const uint64_t b = g / gmax, i0 = (g % gmax) * kNGroup;
    if (b >= a.n_blocks) return;
    const NDecBlock k = a.blocks[b];
    if (!n_sec_ok(a, k)) return;  // (k_n_sums set the status)
    const uint64_t n = k.r1 - k.r0;
    if (i0 >= n) return;
    const uint8_t *sec = a.payload + k.payload_off;
    const uint8_t *mids = sec + 4 * n;
    const uint32_t cnt = (uint32_t)umin(kNGroup, n - i0);
    uint32_t plen = 0, cur = 0;
    for (uint32_t t = 0; t < cnt; t++, cur ^= 1) {
        const uint64_t i = i0 + t, r = k.r0 + i;
        const uint32_t len = a.len[r], pre = sec[2 * n + i], suf = sec[3 * n + i];
        const uint64_t mo = a.mid_off[r] - a.mid_off[k.r0], out = a.name_off[r];
        // (k_n_lens and k_n_sums passed these; no index below leaves its buffer without them)
        if (!n_read_ok(t, len, pre, suf, plen) || mo > k.mid_bytes || len - pre - suf > k.mid_bytes - mo ||
            out > a.names_cap || len > a.names_cap - out) {
            if (lane == 0) n_fail(a.status, r);
            return;
        }
        const uint8_t *p = buf[wave][cur ^ 1];
        uint8_t *c = buf[wave][cur];
        for (uint32_t j = lane; j < len; j += 64) {
            const uint8_t ch = n_byte(p, plen, mids + mo, len, pre, suf, j);
            c[j] = ch;
            a.names[out + j] = ch;
        }
        plen = len;
        __threadfence_block();  // the next name reads this one from LDS (same wave, other lanes)
    }
}

// every size is 0 unless the status is clear (walk, patch, unpack and expand)
__global__ __launch_bounds__(256) void k_named_sizes(const uint64_t *offs, const uint64_t *name_off, uint64_t n,
                                                     uint32_t fastq, const unsigned long long *status, uint64_t *sizes) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t len = offs[r + 1] - offs[r], nlen = name_off[r + 1] - name_off[r];
    sizes[r] = *status != ~0ull ? 0 : fastq ? nlen + 2 * len + 6 : nlen + len + 3;
}

// W: the call has a window (window.hip zeroed the sizes outside it): reads without a record are
// skipped.  W = false is the kernel as it was.
template <bool W>
__global__ __launch_bounds__(256) void k_named(const uint8_t *bases, const uint8_t *quals, const uint64_t *offs,
                                               const uint8_t *names, const uint64_t *name_off, uint64_t n,
                                               const uint64_t *out_offs, uint64_t out_cap, uint8_t *out) {
    if (out_offs[n] == 0 || out_offs[n] > out_cap) return;  // a failed call (sizes 0) or a short buffer
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
    const uint64_t o0 = offs[0];
    for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); r < n; r += waves) {
        if (W && w_skips(out_offs[r], out_offs[r + 1])) continue;
        const uint64_t b = offs[r] - o0, len = offs[r + 1] - offs[r];
        const uint64_t nb = name_off[r], nlen = name_off[r + 1] - nb;
        uint64_t o = out_offs[r];
        if (lane == 0) out[o] = quals ? '@' : '>';
        for (uint64_t i = lane; i < nlen; i += 64) out[o + 1 + i] = names[nb + i];
        if (lane == 0) out[o + 1 + nlen] = '\n';
        o += nlen + 2;
        for (uint64_t i = lane; i < len; i += 64) out[o + i] = bases[b + i];
        if (!quals) {
            if (lane == 0) out[o + len] = '\n';
            continue;
        }
        if (lane < 3) out[o + len + lane] = (uint8_t)"\n+\n"[lane];
        o += len + 3;
        for (uint64_t i = lane; i < len; i += 64) out[o + i] = quals[b + i];
        if (lane == 0) out[o + len] = '\n';
    }
}

}  // namespace

// the columns, every header byte at most once, and each section's padding
uint64_t names_payload_max(uint64_t n_raw, uint64_t n_reads, uint64_t n_blocks) {
    return 4 * n_reads + n_raw + 8 * n_blocks + 8;
}

void launch_names_pack(const NEncArgs &a, hipStream_t s) {
    if (a.n_blocks == 0) return;
    (void)hipMemsetAsync(a.status, 0xFF, 8, s);  // a failure shows in the caller's hipGetLastError
    const uint64_t blocks = std::min<uint64_t>((a.n_reads + 3) / 4, 65536);
    hipLaunchKernelGGL(k_n_measure, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    scan_excl_u32(a.len, a.n_reads, a.len_off, a.tmp, s);
    scan_excl_u32(a.mid, a.n_reads, a.mid_off, a.tmp, s);
    hipLaunchKernelGGL(k_n_blocks, dim3(1), dim3(256), 0, s, a);
    const uint64_t groups = a.n_blocks * ((a.block_reads + kNGroup - 1) / kNGroup);
    hipLaunchKernelGGL(k_n_emit, dim3((uint32_t)((groups + 3) / 4)), dim3(256), 0, s, a);
}

void launch_names_expand(const NDecArgs &a, hipStream_t s) {
    if (a.n_blocks == 0 || a.n_reads == 0) return;
    hipLaunchKernelGGL(k_n_lens, dim3((uint32_t)((a.n_reads + 255) / 256)), dim3(256), 0, s, a);
    scan_excl_u32(a.len, a.n_reads, a.name_off, a.tmp, s);
    scan_excl_u32(a.mid, a.n_reads, a.mid_off, a.tmp, s);
    hipLaunchKernelGGL(k_n_sums, dim3((uint32_t)((a.n_blocks + 255) / 256)), dim3(256), 0, s, a);
    // every section gets the groups of the largest: (b, j) past a section's reads returns
    const uint64_t gmax = (a.max_reads + kNGroup - 1) / kNGroup;
    if (gmax == 0) return;
    hipLaunchKernelGGL(k_n_expand, dim3((uint32_t)((a.n_blocks * gmax + 3) / 4)), dim3(256), 0, s, a, gmax);
}

void launch_named_text(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offs, const uint8_t *d_names,
                       const uint64_t *d_name_off, uint64_t n, const unsigned long long *d_status, uint64_t *sizes,
                       uint64_t *out_offs, uint64_t *tmp, uint8_t *out, uint64_t out_cap, hipStream_t s, uint64_t w_first,
                       uint64_t w_count) {
    if (!n) return;
    hipLaunchKernelGGL(k_named_sizes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_offs, d_name_off, n,
                       d_quals ? 1u : 0u, d_status, sizes);
    if (w_count) launch_window_sizes(sizes, n, w_first, w_count, s);
    scan_excl_u64(sizes, n, out_offs, tmp, s);
    const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, 65536);
    hipLaunchKernelGGL(w_count ? k_named<true> : k_named<false>, dim3((uint32_t)blocks), dim3(256), 0, s, d_bases, d_quals,
                       d_offs, d_names, d_name_off, n, out_offs, out_cap, out);
}

}  // namespace ntc
