// Non-ACGT symbols on the GPU (nonacgt_core.h has the logic, DESIGN.md "Non-ACGT symbols").
// Encode: the staged bases are flagged (one read of the bases), runs of one identical symbol
// are listed in (read, pos) order by prefix sums over the bitmaps, and the flagged bytes are
// rewritten to the substitute base, so k_pack and everything after it see A/C/G/T only.
// Decode: k_nx_patch puts the listed symbols back over the substitute bases.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nonacgt_core.h"

namespace ntc {

namespace {

// Thread t flags chunk t: positions [16 t, 16 t + 16).  One uint4 load per lane (bases +
// offs[0] is 16-byte aligned on the staged buffers; any other start reads bytes); the two
// neighbour bytes are read only when the chunk holds a non-ACGT byte.  Chunks past the
// batch, up to the last word's end, are written as zero.
__global__ __launch_bounds__(256) void k_nx_flag(NxArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * a.n_words) return;
    uint16_t *M16 = reinterpret_cast<uint16_t *>(a.M), *S16 = reinterpret_cast<uint16_t *>(a.S),
             *E16 = reinterpret_cast<uint16_t *>(a.E);
    const uint64_t x0 = t * 16;
    NxFlags f{0, 0, 0};
    if (x0 < a.total) {
        const uint8_t *B = a.bases + a.offs[0];
        const uint32_t n = a.total - x0 < 16 ? (uint32_t)(a.total - x0) : 16u;
        uint32_t w[4] = {0, 0, 0, 0};
        if ((((uintptr_t)B) & 15) == 0 && n == 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(B + x0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; j++)
                if (j < n) w[j >> 2] |= (uint32_t)B[x0 + j] << (8 * (j & 3));
        }
        f = nx_chunk_flags(w, n, kNxNone, kNxNone);  // the flags alone decide whether to look further
        if (f.m) {
            const uint32_t prev = x0 ? B[x0 - 1] : kNxNone;
            const uint32_t next = x0 + 16 < a.total ? B[x0 + 16] : kNxNone;
            f = nx_chunk_flags(w, n, prev, next);
        }
    }
    M16[t] = (uint16_t)f.m;
    S16[t] = (uint16_t)f.s;
    E16[t] = (uint16_t)f.e;
}

// Thread r adds read r's boundary bits: a run starts at a read's first position and ends at
// its last, whatever the neighbouring read holds.  Setting a bit is all the atomic does.
__global__ __launch_bounds__(256) void k_nx_bounds(NxArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint64_t p = a.offs[r] - a.offs[0], q = a.offs[r + 1] - a.offs[0];
    if (q <= p || q > a.total) return;
    unsigned int *S32 = reinterpret_cast<unsigned int *>(a.S), *E32 = reinterpret_cast<unsigned int *>(a.E);
    if (nx_bit(a.M, p) && !nx_bit(a.S, p)) atomicOr(S32 + (p >> 5), 1u << (p & 31));
    if (nx_bit(a.M, q - 1) && !nx_bit(a.E, q - 1)) atomicOr(E32 + ((q - 1) >> 5), 1u << ((q - 1) & 31));
}

// per word: run starts, run ends; the flagged bases go to counts[1] (a sum, block by block)
__global__ __launch_bounds__(256) void k_nx_count(NxArgs a) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t nb = 0;
    if (w < a.n_words) {
        a.cnt_s[w] = (uint32_t)__popcll(a.S[w]);
        a.cnt_e[w] = (uint32_t)__popcll(a.E[w]);
        nb = (uint32_t)__popcll(a.M[w]);
    }
    __shared__ uint32_t sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    if (nb) atomicAdd(&sum, nb);
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long *)(a.counts + 1), (unsigned long long)sum);
}

// counts[0] = runs; a batch whose starts and ends do not pair (never expected) fails
// and both counts into the host mailbox (per-lane addresses: vector stores, as k_status_box)
__global__ __launch_bounds__(64) void k_nx_total(NxArgs a) {
    const uint32_t t = threadIdx.x;
    if (t >= 2) return;
    const uint64_t ns = a.n_words ? a.soff[a.n_words] : 0, ne = a.n_words ? a.eoff[a.n_words] : 0;
    const uint64_t v = t == 0 ? ns : a.counts[1];
    if (t == 0) a.counts[0] = ns;
    a.box[kBoxNxRuns + t] = v;  // then kBoxNxBases
    if (t == 0 && ns != ne) atomicMin(a.status, (unsigned long long)kErrFormat);
}

// Thread i writes run i (those that fit the list; counts[0] tells the host when to come
// back with a larger one).
__global__ __launch_bounds__(256) void k_nx_emit(NxArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t n = a.soff[a.n_words];
    if (i >= n || i >= a.run_cap || n != a.eoff[a.n_words]) return;
    NxRun r;
    if (!nx_emit_run(i, a.S, a.E, a.soff, a.eoff, a.n_words, a.bases, a.offs, a.n_reads, r))
        atomicMin(a.status, (unsigned long long)((r.read << 8) | (uint64_t)kErrLength));
    a.runs[i] = r;
}

// Thread t rewrites the flagged bytes of chunk t to the substitute base.  After k_nx_emit:
// the flag and emit passes read the bytes this one changes.
__global__ __launch_bounds__(256) void k_nx_substitute(NxArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 4 * a.n_words) return;
    uint32_t m = reinterpret_cast<const uint16_t *>(a.M)[t];
    if (!m) return;
    uint8_t *B = a.bases + a.offs[0] + t * 16;
    for (; m; m &= m - 1) B[__builtin_ctz(m)] = (uint8_t)a.sub;
}

constexpr uint32_t kNxLaneMax = 32;  // k_nx_patch: longer pieces take a wave

// Lane i checks piece i (a run, or a slice of a long run cut by the host) and writes its
// symbol over the substitute bases; pieces longer than kNxLaneMax are then taken one by one
// by the whole wave.  A piece that fails a check writes nothing and sets the status.
__global__ __launch_bounds__(256) void k_nx_patch(NxPatchArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    if (*a.status != ~0ull) return;  // the walk failed: offsets and bases are not to be trusted
    NxRun r{0, 0, 0, 0, 0};
    bool ok = false, live = i < a.n;
    if (live) {
        r = a.runs[i];
        ok = nx_run_fits(r, a.offs, a.n_reads);
    }
    uint8_t *p = ok ? a.bases + (a.offs[r.read] - a.offs[0]) + r.pos : nullptr;
    if (ok && r.len <= kNxLaneMax) {
        for (uint32_t j = 0; j < r.len; j++) ok &= p[j] == a.sub;
        if (ok)
            for (uint32_t j = 0; j < r.len; j++) p[j] = (uint8_t)r.sym;
    }
    unsigned long long longs = __ballot(ok && r.len > kNxLaneMax);
    for (; longs; longs &= longs - 1) {
        const int src = __builtin_ctzll(longs);
        const uint32_t len = __shfl(r.len, src), sym = __shfl(r.sym, src);
        const uint64_t mine = ok ? (uint64_t)(p - a.bases) : 0;
        const uint64_t at = (uint64_t)__shfl((uint32_t)mine, src) | (uint64_t)__shfl((uint32_t)(mine >> 32), src) << 32;
        uint8_t *q = a.bases + at;
        bool same = true;
        for (uint32_t j = lane; j < len; j += 64) same &= q[j] == a.sub;
        const bool all = __all(same);
        if (all)
            for (uint32_t j = lane; j < len; j += 64) q[j] = (uint8_t)sym;
        if (lane == (uint32_t)src) ok = all;
    }
    if (live && !ok)
        atomicMin(a.status, (unsigned long long)(((r.read < a.n_reads ? r.read : 0) << 8) | (uint64_t)kErrFormat));
}

static inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

uint64_t nx_words(uint64_t total) { return (total + 63) / 64; }

void launch_nx_mask(const NxArgs &a, uint64_t *scan_tmp, hipStream_t s) {
    (void)hipMemsetAsync(a.counts, 0, 16, s);  // a failure shows in the caller's hipGetLastError
    if (a.n_words == 0) {
        hipLaunchKernelGGL(k_nx_total, dim3(1), dim3(64), 0, s, a);
        return;
    }
    hipLaunchKernelGGL(k_nx_flag, grid_for(4 * a.n_words), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_nx_bounds, grid_for(a.n_reads), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_nx_count, grid_for(a.n_words), dim3(256), 0, s, a);
    scan_excl_u32(a.cnt_s, a.n_words, a.soff, scan_tmp, s);
    scan_excl_u32(a.cnt_e, a.n_words, a.eoff, scan_tmp, s);
    hipLaunchKernelGGL(k_nx_total, dim3(1), dim3(64), 0, s, a);
    if (a.runs && a.run_cap)  // policy keep; one thread per listed run at most
        hipLaunchKernelGGL(k_nx_emit, grid_for(a.run_cap), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_nx_substitute, grid_for(4 * a.n_words), dim3(256), 0, s, a);
}

void launch_nx_patch(const NxPatchArgs &a, hipStream_t s) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_nx_patch, grid_for(a.n), dim3(256), 0, s, a);
}

}  // namespace ntc
